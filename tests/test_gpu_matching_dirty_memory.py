"""The global matching on dirty, guarded memory (tests/dirty_memory.py).

`_matching` allocates its outputs, the matching probability, the workspace of the backward (28 bytes a pixel) and the gradients with
`torch.empty` under its own module-level name `torch`; here that name is a `dirty_memory.Harness` proxy, so every such tensor is carved out
of a buffer  guard | body | guard  whose body holds the fill byte.  For the forward with and without prob, for the whole backward and for
either gradient alone: the same bits under the fills 0x00, 0xFF and 0x55 (nothing stale is read: every element of every output and every
byte of the workspace is written before it is read), no guard of any allocation is written, the inputs -- guarded copies, their guards
holding the fill byte; the workspace among them in the backward -- are unchanged, and every allocation is made by a function of the new
module."""
import numpy as np
import pytest
import torch

import dirty_memory as dm
import matching_oracle as mo

pytestmark = pytest.mark.gpu

FRAMES = [(3, 5, 7), (2, 5, 13)]                     # Q = 35, narrower than a wave; Q = 65: two p-tiles and three q-chunks
C = 5


def _run(fill, n, h, w, what):
    from oflibpytorch_amd import _matching
    dev = torch.device('cuda', 0)
    feat, other = (torch.from_numpy(x.copy()).to(dev) for x in mo.features_general(n, C, h, w))
    g = torch.from_numpy(mo.upstream(n, h, w).copy()).to(dev)
    stats = _matching.flow_global_match(feat, other, -1.0, False, True)[2]                   # (made ahead: an input of the backward)
    harness = dm.Harness(fill)
    feat, other, g, stats = harness.guard_all(feat, other, g, stats)
    assert _matching.torch is torch
    _matching.torch = harness.proxy
    try:
        if what == "forward":
            res = list(_matching.flow_global_match(feat, other, -1.0, True, True))
            allocations, callers = 3, ["flow_global_match"]                                   # the vectors, prob, the workspace
        elif what == "forward-no-prob":
            res = [_matching.flow_global_match(feat, other, -1.0, False, False)[0]]
            allocations, callers = 1, ["flow_global_match"]
        elif what == "grads":
            res = list(_matching.flow_global_match_grad(feat, other, -1.0, stats, g))
            allocations, callers = 2, ["flow_global_match_grad"]                              # d feat, d other
        elif what == "grad-feat":
            res = [_matching.flow_global_match_grad(feat, other, -1.0, stats, g, want_other=False)[0]]
            allocations, callers = 1, ["flow_global_match_grad"]
        else:
            res = [_matching.flow_global_match_grad(feat, other, -1.0, stats, g, want_feat=False)[1]]
            allocations, callers = 1, ["flow_global_match_grad"]
        torch.cuda.synchronize()
    finally:
        _matching.torch = torch
    assert harness.callers() == callers
    assert len(harness.log) == allocations
    harness.check_guards()
    harness.check_inputs_unchanged()
    return res


@pytest.mark.parametrize("what", ["forward", "forward-no-prob", "grads", "grad-feat", "grad-other"])
@pytest.mark.parametrize("n,h,w", FRAMES)
def test_same_bits_under_every_fill(n, h, w, what):
    results = [_run(fill, n, h, w, what) for fill in dm.FILLS]
    for fill, res in zip(dm.FILLS[1:], results[1:]):
        dm.assert_same_bits(res, results[0], "%s under fill 0x%02X against 0x00" % (what, fill))
    feat, other = mo.features_general(n, C, h, w)                                             # ... and they are the right ones
    q = h * w
    if what.startswith("forward"):
        r = mo.compute(feat, other, -1.0)
        want = [(r['out'], r['mag'], mo.forward_shift(q))]
    else:
        r = mo.grads(feat, other, -1.0, mo.upstream(n, h, w))
        both = [(r['d_feat64'], r['mag_feat'], mo.grad_shift(q)), (r['d_other64'], r['mag_other'], mo.grad_shift(q))]
        want = {"grads": both, "grad-feat": both[:1], "grad-other": both[1:]}[what]
    for got, (exp, mag, shift) in zip(results[0], want):
        got = got.cpu().numpy()
        assert got.dtype == np.float32 and np.all(np.abs(got - exp) <= mo.ulp32(exp) + 2.0 ** -shift * mag)
