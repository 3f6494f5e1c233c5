"""Flow.corr_lookup on dirty, guarded memory (tests/dirty_memory.py).

`_corr_lookup` allocates its outputs, the workspace of the backward (the node gradients Gn) and the keys with `torch.empty` under its own
module-level name `torch`; here that name is a `dirty_memory.Harness` proxy, so every such tensor is carved out of a buffer
guard | body | guard  whose body holds the fill byte.  For the lookup (one launch per level into one result), for the whole backward (per
level: the nodes pass, d feat continuing the stored sums, the gather of d other) and for either gradient alone: the same bits under the
fills 0x00, 0xFF and 0x55 (nothing stale is read -- the sums d feat continues are those the level before stored -- and every element of
every output, of the workspace and of the keys is written before it is read), no guard of any allocation is written, the inputs --
guarded copies, their guards holding the fill byte -- are unchanged, and every allocation is made by a function of the new module."""
import numpy as np
import pytest
import torch

import corr_lookup_oracle as cl
import dirty_memory as dm

pytestmark = pytest.mark.gpu

FRAMES = [(3, 5, 7), (2, 9, 33)]                     # narrower than a tile row and than the window; 2 x 2 tiles per image


def _run(fill, n, h, w, ref, what, half, radius, c):
    from oflibpytorch_amd import _corr_lookup
    dev = torch.device('cuda', 0)
    a, m = (torch.from_numpy(x.copy()).to(dev) for x in cl.case(n, h, w, ref))
    feat, lv = cl.explicit_levels(n, c, h, w, ref)
    feat, lv = torch.from_numpy(feat.copy()).to(dev), [torch.from_numpy(x.copy()).to(dev) for x in lv]
    g = torch.from_numpy(cl.upstream(n, 4 * (2 * radius + 1) ** 2, h, w).copy()).to(dev)
    if half:
        a = a.half()
    harness = dm.Harness(fill)
    a, m, feat, g = harness.guard_all(a, m, feat, g)
    lv = list(harness.guard_all(*lv))
    assert _corr_lookup.torch is torch
    _corr_lookup.torch = harness.proxy
    try:
        if what == "lookup":
            res = [_corr_lookup.flow_corr_lookup(a, m, feat, lv, cl.sign_of(ref), radius)]
            allocations, callers = 1, ["flow_corr_lookup"]
        elif what == "grads":
            d_feat, d_levels = _corr_lookup.flow_corr_lookup_grad(a, m, feat, lv, cl.sign_of(ref), radius, g)
            res = [d_feat] + d_levels
            allocations, callers = 3 + 4, ["flow_corr_lookup_grad"]                           # the workspace, the keys, d feat, four d other
        elif what == "grad-feat":
            res = [_corr_lookup.flow_corr_lookup_grad(a, m, feat, lv, cl.sign_of(ref), radius, g, want_levels=[False] * 4)[0]]
            allocations, callers = 2, ["flow_corr_lookup_grad"]                               # the workspace, d feat
        else:
            d_levels = _corr_lookup.flow_corr_lookup_grad(a, m, feat, lv, cl.sign_of(ref), radius, g, want_feat=False,
                                                          want_levels=[False, True, False, True])[1]
            assert d_levels[0] is None and d_levels[2] is None
            res = [d_levels[1], d_levels[3]]
            allocations, callers = 2 + 2, ["flow_corr_lookup_grad"]                           # the workspace, the keys, two d other
        torch.cuda.synchronize()
    finally:
        _corr_lookup.torch = torch
    assert harness.callers() == callers
    assert len(harness.log) == allocations
    harness.check_guards()
    harness.check_inputs_unchanged()
    return res


@pytest.mark.parametrize("half,radius,c", [(False, 4, 9), (True, 1, 3)], ids=["fp32-radius4", "fp16-radius1"])
@pytest.mark.parametrize("what", ["lookup", "grads", "grad-feat", "grad-levels"])
@pytest.mark.parametrize("ref", cl.REFS)
@pytest.mark.parametrize("n,h,w", FRAMES)
def test_same_bits_under_every_fill(n, h, w, ref, what, half, radius, c):
    results = [_run(fill, n, h, w, ref, what, half, radius, c) for fill in dm.FILLS]
    for fill, res in zip(dm.FILLS[1:], results[1:]):
        dm.assert_same_bits(res, results[0], "%s under fill 0x%02X against 0x00" % (what, fill))
    a, m = cl.case(n, h, w, ref)                                                              # ... and they are the right ones
    feat, lv = cl.explicit_levels(n, c, h, w, ref)                                            # (the fp16-stored flow holds the same vectors)
    if what == "lookup":
        want = [cl.compute(a, m, feat, lv, ref, radius)['lookup']]
    else:
        d_feat, d_levels = cl.grads(a, m, feat, lv, ref, radius, cl.upstream(n, 4 * (2 * radius + 1) ** 2, h, w))
        want = {"grads": [d_feat] + d_levels, "grad-feat": [d_feat], "grad-levels": [d_levels[1], d_levels[3]]}[what]
    assert len(want) == len(results[0])
    for got, exp in zip(results[0], want):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), exp.view(np.uint32))
