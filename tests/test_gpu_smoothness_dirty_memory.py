"""Flow.smoothness / smoothness_map / smoothness_stats on dirty, guarded memory (tests/dirty_memory.py).

`_smoothness` allocates its outputs and its workspace with `torch.empty` under its own module-level name `torch`; here that name is a
`dirty_memory.Harness` proxy, so every such tensor is carved out of a buffer  guard | body | guard  whose body holds the fill byte.  For
the records, the map and the forward plus backward pass: the same bits under the fills 0x00, 0xFF and 0x55 (nothing stale is read: not
the workspace, not an output), no guard of any allocation is written, the inputs -- guarded copies, their guards holding the fill byte
-- are unchanged, and every allocation is made by a function of the new module."""
import numpy as np
import pytest
import torch

import dirty_memory as dm
import smoothness_oracle as so

pytestmark = pytest.mark.gpu

FRAMES = [(3, 5, 7), (3, 37, 53)]                    # the scalar form; 5 blocks per image
ALPHA, EPS = 10.0, 1e-3


def _run(fill, n, h, w, order, what, kind, half):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _smoothness
    dev = torch.device('cuda', 0)
    f, m = (torch.from_numpy(a.copy()).to(dev) for a in so.case(n, h, w))
    img = None if kind is None else torch.from_numpy(so.image(n, h, w, 3, kind == "u8").copy()).to(dev)
    if half:
        f = f.half()
    harness = dm.Harness(fill)
    f, m, img = harness.guard_all(f, m, img)
    assert _smoothness.torch is torch
    _smoothness.torch = harness.proxy
    try:
        if what == "stats":
            res = list(_smoothness.flow_smoothness(f, m, img, order, ALPHA, EPS))
            allocations, callers = 2, ["flow_smoothness"]
        elif what == "map":
            res = list(_smoothness.flow_smoothness(f, m, img, order, ALPHA, EPS, want_map=True))
            allocations, callers = 3, ["flow_smoothness"]
        else:
            f.requires_grad_(True)
            loss = ofl.Flow(f, 't', m).smoothness(img, order=order, alpha=ALPHA, eps=EPS)
            (loss * torch.tensor(so.UPSTREAM, device=dev)).sum().backward()
            res = [loss.detach(), f.grad]
            allocations, callers = 3, ["flow_smoothness", "flow_smoothness_grad"]
        torch.cuda.synchronize()
    finally:
        _smoothness.torch = torch
    assert harness.callers() == callers
    assert len(harness.log) == allocations
    harness.check_guards()
    harness.check_inputs_unchanged()
    return res


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("kind", [None, "f32", "u8"], ids=["plain", "f32", "u8"])
@pytest.mark.parametrize("what", ["stats", "map", "backward"])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("n,h,w", FRAMES)
def test_same_bits_under_every_fill(n, h, w, order, what, kind, half):
    results = [_run(fill, n, h, w, order, what, kind, half) for fill in dm.FILLS]
    for fill, res in zip(dm.FILLS[1:], results[1:]):
        dm.assert_same_bits(res, results[0], "%s under fill 0x%02X against 0x00" % (what, fill))
    if what != "backward" and kind is None and not half:                     # ... and they are the right bits
        want = so.compute(*so.case(n, h, w), None, order, ALPHA, EPS)
        rec = results[0][0].cpu().numpy()
        assert np.array_equal(rec[:, :2], want['records'][:, :2]) and np.array_equal(rec[:, 4], want['records'][:, 4])
        assert not rec[:, 5:].any()
        if what == "map":
            assert np.array_equal(results[0][1].cpu().numpy().view(np.uint32), want['map'].view(np.uint32))
