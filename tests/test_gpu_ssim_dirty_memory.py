"""Flow.ssim / ssim_map / ssim_stats on dirty, guarded memory (tests/dirty_memory.py).

`_ssim` allocates its outputs and its workspace with `torch.empty` under its own module-level name `torch`; here that name is a
`dirty_memory.Harness` proxy, so every such tensor is carved out of a buffer  guard | body | guard  whose body holds the fill byte.  For
the records, the map and the forward plus backward pass: the same bits under the fills 0x00, 0xFF and 0x55 (nothing stale is read: not
the workspace, not an output), no guard of any allocation is written, the inputs -- guarded copies, their guards holding the fill byte
-- are unchanged, and every allocation is made by a function of the new module."""
import numpy as np
import pytest
import torch

import dirty_memory as dm
import photometric_oracle as po
import ssim_oracle as so

pytestmark = pytest.mark.gpu

FRAMES = [(3, 5, 7), (3, 37, 53)]                    # narrower than a tile row; 3 x 1 tiles per image


def _run(fill, n, h, w, ref, what, kind, half, window):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _ssim
    dev = torch.device('cuda', 0)
    a, m = (torch.from_numpy(x.copy()).to(dev) for x in po.case(n, h, w, ref)[:2])
    img, other = (torch.from_numpy(x.copy()).to(dev) for x in po.images(n, h, w, ref, kind))
    if half:
        a = a.half()
    harness = dm.Harness(fill)
    a, m, img, other = harness.guard_all(a, m, img, other)
    assert _ssim.torch is torch
    _ssim.torch = harness.proxy
    try:
        if what == "stats":
            res = list(_ssim.flow_ssim(a, m, img, other, so.sign_of(ref), window))
            allocations, callers = 2, ["flow_ssim"]
        elif what == "map":
            res = list(_ssim.flow_ssim(a, m, img, other, so.sign_of(ref), window, want_map=True, want_record=False))
            allocations, callers = 1, ["flow_ssim"]
        else:
            a.requires_grad_(True)
            loss = ofl.Flow(a, ref, m).ssim(img, other, window=window)
            loss.backward(torch.tensor(so.UPSTREAM, device=dev))
            res = [loss.detach(), a.grad]
            allocations, callers = 3, ["flow_ssim", "flow_ssim_grad"]
        torch.cuda.synchronize()
    finally:
        _ssim.torch = torch
    assert harness.callers() == callers
    assert len(harness.log) == allocations
    harness.check_guards()
    harness.check_inputs_unchanged()
    return res


@pytest.mark.parametrize("half,window", [(False, 7), (True, 3)], ids=["fp32-window7", "fp16-window3"])
@pytest.mark.parametrize("kind", ["f32c3", "u8c3"])
@pytest.mark.parametrize("what", ["stats", "map", "backward"])
@pytest.mark.parametrize("ref", so.REFS)
@pytest.mark.parametrize("n,h,w", FRAMES)
def test_same_bits_under_every_fill(n, h, w, ref, what, kind, half, window):
    results = [_run(fill, n, h, w, ref, what, kind, half, window) for fill in dm.FILLS]
    for fill, res in zip(dm.FILLS[1:], results[1:]):
        dm.assert_same_bits(res, results[0], "%s under fill 0x%02X against 0x00" % (what, fill))
    if what != "backward" and not half:                                      # ... and they are the right ones
        a, m = po.case(n, h, w, ref)[:2]
        want = so.compute(a, m, *po.images(n, h, w, ref, kind), ref, window)
        if what == "stats":
            rec = results[0][0].cpu().numpy()
            assert np.array_equal(rec[:, 0], want['records'][:, 0]) and np.array_equal(rec[:, 3], want['records'][:, 3])
            assert np.array_equal(rec[:, 2], want['records'][:, 2]) and not rec[:, 4:].any() and results[0][1] is None
        else:
            assert results[0][0] is None
            got = results[0][1].cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want['map'].view(np.uint32))
