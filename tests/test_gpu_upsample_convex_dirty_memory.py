"""Flow.upsample_convex on dirty, guarded memory (tests/dirty_memory.py).

`_upsample` allocates its outputs and the workspace of the backward (the maximum and the sum of every fine pixel's softmax, float64) with
`torch.empty` under its own module-level name `torch`; here that name is a `dirty_memory.Harness` proxy, so every such tensor is carved
out of a buffer  guard | body | guard  whose body holds the fill byte.  For the forward with and without a mask, for the whole backward and
for either gradient alone: the same bits under the fills 0x00, 0xFF and 0x55 (nothing stale is read: every element of every output, of the
mask block and of the workspace is written before it is read), no guard of any allocation is written, the inputs -- guarded copies, their
guards holding the fill byte -- are unchanged, and every allocation is made by a function of the new module."""
import numpy as np
import pytest
import torch

import dirty_memory as dm
import upsample_convex_oracle as uo

pytestmark = pytest.mark.gpu

FRAMES = [(3, 5, 7), (2, 3, 70)]                     # narrower than a wave; 2 tiles along x and 2 or more blocks of fine rows per image


def _run(fill, n, h, w, k, what, half):
    from oflibpytorch_amd import _upsample
    dev = torch.device('cuda', 0)
    f, m = (torch.from_numpy(x.copy()).to(dev) for x in uo.case(n, h, w))
    lg = torch.from_numpy(uo.logits_general(n, k, h, w).copy()).to(dev)
    g = torch.from_numpy(uo.upstream(n, k, h, w).copy()).to(dev)
    if half:
        f = f.half()
    harness = dm.Harness(fill)
    f, m, lg, g = harness.guard_all(f, m, lg, g)
    assert _upsample.torch is torch
    _upsample.torch = harness.proxy
    try:
        if what == "forward":
            res = list(_upsample.flow_upsample_convex(f, m, lg, k))
            allocations, callers = 2, ["flow_upsample_convex"]                                # the result and its mask
        elif what == "forward-no-mask":
            res = [_upsample.flow_upsample_convex(f, None, lg, k)[0]]
            allocations, callers = 1, ["flow_upsample_convex"]
        elif what == "grads":
            res = list(_upsample.flow_upsample_convex_grad(f, lg, k, g))
            allocations, callers = 3, ["flow_upsample_convex_grad"]                           # d logits, d vecs, the workspace
        elif what == "grad-logits":
            res = [_upsample.flow_upsample_convex_grad(f, lg, k, g, want_vecs=False)[0]]
            allocations, callers = 1, ["flow_upsample_convex_grad"]
        else:
            res = [_upsample.flow_upsample_convex_grad(f, lg, k, g, want_logits=False)[1]]
            allocations, callers = 2, ["flow_upsample_convex_grad"]                           # d vecs, the workspace
        torch.cuda.synchronize()
    finally:
        _upsample.torch = torch
    assert harness.callers() == callers
    assert len(harness.log) == allocations
    harness.check_guards()
    harness.check_inputs_unchanged()
    dm.assert_bool_bytes(res, what)
    return res


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("what", ["forward", "forward-no-mask", "grads", "grad-logits", "grad-vecs"])
@pytest.mark.parametrize("k", uo.FACTORS)
@pytest.mark.parametrize("n,h,w", FRAMES)
def test_same_bits_under_every_fill(n, h, w, k, what, half):
    results = [_run(fill, n, h, w, k, what, half) for fill in dm.FILLS]
    for fill, res in zip(dm.FILLS[1:], results[1:]):
        dm.assert_same_bits(res, results[0], "%s under fill 0x%02X against 0x00" % (what, fill))
    f, m = uo.case(n, h, w)                                                                   # ... and they are the right ones
    lg, g = uo.logits_general(n, k, h, w), uo.upstream(n, k, h, w)                            # (the fp16-stored flow holds the same vectors)
    if what.startswith("forward"):
        r = uo.compute(f, lg, k, float64=True)
        want = [(r['out'], r['mag'], 44)]
        if what == "forward":
            assert np.array_equal(results[0][1].cpu().numpy(), uo.mask_of(m, k))
    else:
        r = uo.grads(f, lg, k, g, float64=True)
        both = [(r['d_logits'], r['mag_logits'], 40), (r['d_flow'], r['mag_flow'], 40)]
        want = {"grads": both, "grad-logits": both[:1], "grad-vecs": both[1:]}[what]
    for got, (exp, mag, shift) in zip(results[0], want):
        got = got.cpu().numpy()
        assert got.dtype == np.float32 and np.all(np.abs(got - exp) <= uo.ulp32(exp) + 2.0 ** -shift * mag)
