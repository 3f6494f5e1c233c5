"""Flow.census / census_map / census_stats on dirty, guarded memory (tests/dirty_memory.py).

`_census` allocates its outputs and its workspace with `torch.empty` under its own module-level name `torch`; here that name is a
`dirty_memory.Harness` proxy, so every such tensor is carved out of a buffer  guard | body | guard  whose body holds the fill byte.  For
the records, the map and the forward plus backward pass: the same bits under the fills 0x00, 0xFF and 0x55 (nothing stale is read: not
the workspace, not an output), no guard of any allocation is written, the inputs -- guarded copies, their guards holding the fill byte
-- are unchanged, and every allocation is made by a function of the new module."""
import numpy as np
import pytest
import torch

import census_oracle as cen
import dirty_memory as dm
import photometric_oracle as po

pytestmark = pytest.mark.gpu

FRAMES = [(3, 5, 7), (3, 37, 53)]                    # narrower than a tile row; 3 x 1 tiles per image


def _run(fill, n, h, w, ref, what, kind, half, patch):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _census
    dev = torch.device('cuda', 0)
    a, m = (torch.from_numpy(x.copy()).to(dev) for x in po.case(n, h, w, ref)[:2])
    img, other = (torch.from_numpy(x.copy()).to(dev) for x in po.images(n, h, w, ref, kind))
    if half:
        a = a.half()
    harness = dm.Harness(fill)
    a, m, img, other = harness.guard_all(a, m, img, other)
    assert _census.torch is torch
    _census.torch = harness.proxy
    try:
        if what == "stats":
            res = list(_census.flow_census(a, m, img, other, cen.sign_of(ref), patch))
            allocations, callers = 2, ["flow_census"]
        elif what == "map":
            res = list(_census.flow_census(a, m, img, other, cen.sign_of(ref), patch, want_map=True, want_record=False))
            allocations, callers = 1, ["flow_census"]
        else:
            a.requires_grad_(True)
            loss = ofl.Flow(a, ref, m).census(img, other, patch=patch)
            loss.backward(torch.tensor(cen.UPSTREAM, device=dev))
            res = [loss.detach(), a.grad]
            allocations, callers = 3, ["flow_census", "flow_census_grad"]
        torch.cuda.synchronize()
    finally:
        _census.torch = torch
    assert harness.callers() == callers
    assert len(harness.log) == allocations
    harness.check_guards()
    harness.check_inputs_unchanged()
    return res


@pytest.mark.parametrize("half,patch", [(False, 7), (True, 3)], ids=["fp32-patch7", "fp16-patch3"])
@pytest.mark.parametrize("kind", ["f32c3", "u8c3"])
@pytest.mark.parametrize("what", ["stats", "map", "backward"])
@pytest.mark.parametrize("ref", cen.REFS)
@pytest.mark.parametrize("n,h,w", FRAMES)
def test_same_bits_under_every_fill(n, h, w, ref, what, kind, half, patch):
    results = [_run(fill, n, h, w, ref, what, kind, half, patch) for fill in dm.FILLS]
    for fill, res in zip(dm.FILLS[1:], results[1:]):
        dm.assert_same_bits(res, results[0], "%s under fill 0x%02X against 0x00" % (what, fill))
    if what != "backward" and not half:                                      # ... and they are the right ones
        a, m = po.case(n, h, w, ref)[:2]
        want = cen.compute(a, m, *po.images(n, h, w, ref, kind), ref, patch)
        if what == "stats":
            rec = results[0][0].cpu().numpy()
            assert np.array_equal(rec[:, 0], want['records'][:, 0]) and np.array_equal(rec[:, 3], want['records'][:, 3])
            assert not rec[:, 4:].any() and results[0][1] is None
        else:
            assert results[0][0] is None
            got = results[0][1].cpu().numpy()
            assert not got[~want['known']].view(np.uint32).any()
            assert np.all(np.abs(got.astype(np.float64) - want['map']) <= cen.ulp32(want['map']))
