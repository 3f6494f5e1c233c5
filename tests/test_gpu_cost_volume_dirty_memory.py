"""Flow.cost_volume on dirty, guarded memory (tests/dirty_memory.py).

`_cost_volume` allocates its outputs with `torch.empty` under its own module-level name `torch`; here that name is a
`dirty_memory.Harness` proxy, so every such tensor is carved out of a buffer  guard | body | guard  whose body holds the fill byte.  For
the volume, for both gradient kernels and for the two per-pixel kernels of the backward (the chain vectors, a buffer of their own, and
the select of d flow, which works in place and allocates nothing): the same bits under the fills 0x00, 0xFF and 0x55 (nothing stale is read, every element of
every output is written), no guard of any allocation is written, the inputs -- guarded copies, their guards holding the fill byte -- are
unchanged, and every allocation is made by a function of the new module.  The kernels have no workspace."""
import numpy as np
import pytest
import torch

import cost_volume_oracle as cv
import dirty_memory as dm

pytestmark = pytest.mark.gpu

FRAMES = [(3, 5, 7), (2, 17, 33)]                    # narrower than a tile row and than the window; 2 x 2 tiles per image


def _run(fill, n, h, w, ref, what, half, radius, c):
    from oflibpytorch_amd import _cost_volume
    dev = torch.device('cuda', 0)
    a, m = (torch.from_numpy(x.copy()).to(dev) for x in cv.case(n, h, w, ref))
    feat, other = (torch.from_numpy(x.copy()).to(dev) for x in cv.features(n, c, h, w, ref))
    g = torch.from_numpy(cv.upstream(n, (2 * radius + 1) ** 2, h, w).copy()).to(dev)
    if half:
        a = a.half()
    harness = dm.Harness(fill)
    a, m, feat, other, g = harness.guard_all(a, m, feat, other, g)
    assert _cost_volume.torch is torch
    _cost_volume.torch = harness.proxy
    try:
        if what == "volume":
            res = [_cost_volume.flow_cost_volume(a, m, feat, other, cv.sign_of(ref), radius)]
            allocations, callers = 1, ["flow_cost_volume"]
        elif what == "grads":
            res = list(_cost_volume.flow_cost_volume_grad(a, m, feat, other, cv.sign_of(ref), radius, g))
            allocations, callers = 2, ["flow_cost_volume_grad"]
        elif what == "grad-warped":
            res = [_cost_volume.flow_cost_volume_grad(a, m, feat, other, cv.sign_of(ref), radius, g, want_feat=False)[1]]
            allocations, callers = 1, ["flow_cost_volume_grad"]
        elif what == "chain":
            res = [_cost_volume.flow_cost_volume_chain(a, cv.sign_of(ref))]
            allocations, callers = 1, ["flow_cost_volume_chain"]
        else:
            # the select of d flow works in place on a gradient it is handed and allocates nothing: the gradient is a guarded
            # allocation of this function, filled with finite values
            gf = harness.proxy.empty((n, 2, h, w), dtype=torch.float32, device=dev)
            gf.copy_(torch.from_numpy(cv.upstream(n, 2, h, w).copy()))
            res = [_cost_volume.flow_cost_volume_gate(a, m, cv.sign_of(ref), gf)]
            assert res[0] is gf
            allocations, callers = 1, ["_run"]
        torch.cuda.synchronize()
    finally:
        _cost_volume.torch = torch
    assert harness.callers() == callers
    assert len(harness.log) == allocations
    harness.check_guards()
    harness.check_inputs_unchanged()
    return res


@pytest.mark.parametrize("half,radius,c", [(False, 4, 17), (True, 1, 3)], ids=["fp32-radius4", "fp16-radius1"])
@pytest.mark.parametrize("what", ["volume", "grads", "grad-warped", "chain", "gate"])
@pytest.mark.parametrize("ref", cv.REFS)
@pytest.mark.parametrize("n,h,w", FRAMES)
def test_same_bits_under_every_fill(n, h, w, ref, what, half, radius, c):
    results = [_run(fill, n, h, w, ref, what, half, radius, c) for fill in dm.FILLS]
    for fill, res in zip(dm.FILLS[1:], results[1:]):
        dm.assert_same_bits(res, results[0], "%s under fill 0x%02X against 0x00" % (what, fill))
    if not half:                                                             # ... and they are the right ones
        a, m = cv.case(n, h, w, ref)
        feat, other = cv.features(n, c, h, w, ref)
        if what == "volume":
            want = [cv.compute(a, m, feat, other, ref, radius)['volume']]
        elif what == "chain":
            want = [cv.chain_vectors(a, ref)]
            assert np.array_equal(want[0], a)                                # (finite vectors: the flow's own)
        elif what == "gate":
            usable = cv.usable_of(a, m, ref)
            want = [np.where(usable[:, None], cv.upstream(n, 2, h, w), np.float32(0.0)).astype(np.float32)]
            assert 0.1 < usable.mean() < 0.9
        else:
            want = list(cv.grads(a, m, feat, other, ref, radius, cv.upstream(n, (2 * radius + 1) ** 2, h, w)))[-len(results[0]):]
        for got, exp in zip(results[0], want):
            assert np.array_equal(got.cpu().numpy().view(np.uint32), exp.view(np.uint32))
