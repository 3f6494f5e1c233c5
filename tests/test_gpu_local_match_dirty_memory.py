"""The local matching on dirty, guarded memory (tests/dirty_memory.py).

`_local_match` allocates its outputs, the probability, the statistics of the backward (28 bytes a pixel), the workspace of the backward
and the gradients with `torch.empty` under its own module-level name `torch`; here that name is a `dirty_memory.Harness` proxy, so every
such tensor is carved out of a buffer  guard | body | guard  whose body holds the fill byte.  For the forward with and without
probability and statistics, for both gathers together and for each alone: the same bits under the fills 0x00, 0xFF and 0x55 (nothing
stale is read: every element of every output, every byte of the statistics and every element of the workspace is written before it is
read), no guard of any allocation is written, the inputs -- guarded copies, their guards holding the fill byte; the statistics among them
in the backward -- are unchanged, and every allocation is made by a function of the new module."""
import numpy as np
import pytest
import torch

import dirty_memory as dm
import local_match_oracle as lo

pytestmark = pytest.mark.gpu

FRAMES = [(3, 5, 7), (2, 9, 35)]                     # narrower than a tile; two tiles a row and three rows of tiles of the forward
C = 5
WHATS = ["forward", "forward-bare", "grads", "grad-feat", "grad-warped"]


def _run(fill, n, h, w, radius, ref, what):
    from oflibpytorch_amd import _local_match
    dev = torch.device('cuda', 0)
    sign = lo.sign_of(ref)
    feat, other = (torch.from_numpy(x.copy()).to(dev) for x in lo.features_general(n, C, h, w))
    flow = torch.from_numpy(lo.vectors_general(n, h, w).copy()).to(dev)
    g = torch.from_numpy(lo.upstream(n, h, w).copy()).to(dev)
    mask = torch.from_numpy(lo.masks(n, h, w)['checker'].copy()).to(dev)
    stats = _local_match.flow_local_match(flow, mask, feat, other, sign, radius, False, True)[2]      # (made ahead: an input of the backward)
    harness = dm.Harness(fill)
    flow, mask, feat, other, g, stats = harness.guard_all(flow, mask, feat, other, g, stats)
    assert _local_match.torch is torch
    _local_match.torch = harness.proxy
    try:
        if what == "forward":
            res = list(_local_match.flow_local_match(flow, mask, feat, other, sign, radius, True, True))
            allocations, callers = 3, ["flow_local_match"]                                   # the vectors, the probability, the statistics
        elif what == "forward-bare":
            res = [_local_match.flow_local_match(flow, None, feat, other, sign, radius, False, False)[0]]
            allocations, callers = 1, ["flow_local_match"]
        else:
            wants = {"grads": (True, True), "grad-feat": (True, False), "grad-warped": (False, True)}[what]
            res = [d for d in _local_match.flow_local_match_grad(flow, mask, feat, other, sign, radius, stats, g, *wants) if d is not None]
            allocations, callers = sum(wants) + 1, ["flow_local_match_grad"]                  # ... and the workspace
        torch.cuda.synchronize()
    finally:
        _local_match.torch = torch
    assert harness.callers() == callers
    assert len(harness.log) == allocations
    harness.check_guards()
    harness.check_inputs_unchanged()
    return res


@pytest.mark.parametrize("what", WHATS)
@pytest.mark.parametrize("radius,ref", [(1, 's'), (4, 't')])
@pytest.mark.parametrize("n,h,w", FRAMES)
def test_same_bits_under_every_fill(n, h, w, radius, ref, what):
    results = [_run(fill, n, h, w, radius, ref, what) for fill in dm.FILLS]
    for fill, res in zip(dm.FILLS[1:], results[1:]):
        dm.assert_same_bits(res, results[0], "%s under fill 0x%02X against 0x00" % (what, fill))
    feat, other = lo.features_general(n, C, h, w)                                             # ... and they are the right ones
    flow, g = lo.vectors_general(n, h, w), lo.upstream(n, h, w)
    mask = None if what == "forward-bare" else lo.masks(n, h, w)['checker']
    fwd = lo.compute(flow, mask, feat, other, ref, radius)
    if what.startswith("forward"):
        want = [(fwd['out'], fwd['mag'], lo.forward_shift(fwd['terms'])[:, None])]
        if what == "forward":
            assert np.abs(results[0][1].cpu().numpy().astype(np.float64) - 1.0 / fwd['S']).max() <= 2.0 ** -22
    else:
        r = lo.grads(flow, mask, feat, other, ref, radius, g, res=fwd)
        every = [(r[k + '64'], r['mag_' + k], lo.grad_shift(r['terms_' + k])) for k in ('d_feat', 'd_w')]
        want = {"grads": every, "grad-feat": every[:1], "grad-warped": every[1:]}[what]
    for got, (exp, mag, shift) in zip(results[0], want):
        got = got.cpu().numpy()
        assert got.dtype == np.float32 and np.all(np.abs(got - exp) <= lo.ulp32(exp) + 2.0 ** -np.asarray(shift, np.float64) * mag)
