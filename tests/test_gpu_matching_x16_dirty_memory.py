"""The global matching of fp16 / bf16 features on dirty, guarded memory (tests/dirty_memory.py).

`_matching` allocates the vectors, the matching probability, the statistics of the backward and the packed rows of the 16-bit route with
`torch.empty` under its own module-level name `torch`; here that name is a `dirty_memory.Harness` proxy, so every such tensor is carved out
of a buffer  guard | body | guard  whose body holds the fill byte.  For the forward with and without prob and statistics, in both dtypes,
with channels that need padding (C = 5 of 16; C = 130 of 144, the instantiation that reloads the pixels' fragments) and frames whose last
chunk and last tile are partial: the same bits under the fills 0x00, 0xFF and 0x55 -- nothing stale is read: the packed rows, their padded
channels and padded rows are all written before the walk reads them, and the walk's padded positions take no part --, no guard of any
allocation is written, the inputs -- guarded copies, their guards holding the fill byte -- are unchanged, and every allocation is made
by the new binding.  The backward is the float32 route's, on the statistics this forward leaves: run once on them, in dirty memory too."""
import numpy as np
import pytest
import torch

import dirty_memory as dm
import matching_oracle as mo
import matching_x16_oracle as xo

pytestmark = pytest.mark.gpu

CASES = [(3, 5, 5, 7), (2, 5, 5, 13), (1, 130, 3, 11)]       # (n, C, h, w): Q = 35; Q = 65: two tiles, three chunks; C beyond the registers
NAMES = ('fp16', 'bf16')


def _run(fill, name, n, c, h, w, what):
    from oflibpytorch_amd import _matching
    dev = torch.device('cuda', 0)
    f16, o16, _, _ = xo.features_general(name, n, c, h, w)
    g = torch.from_numpy(mo.upstream(n, h, w).copy()).to(dev)
    harness = dm.Harness(fill)
    feat, other, g = harness.guard_all(f16.to(dev), o16.to(dev), g)
    assert _matching.torch is torch
    _matching.torch = harness.proxy
    try:
        if what == "forward":
            res = list(_matching.flow_global_match_x16(feat, other, -1.0, True, True))
            allocations, callers = 4, ["flow_global_match_x16"]                               # the vectors, prob, the statistics, the packed rows
        elif what == "forward-bare":
            res = [_matching.flow_global_match_x16(feat, other, -1.0, False, False)[0]]
            allocations, callers = 2, ["flow_global_match_x16"]
        else:
            out, _, stats = _matching.flow_global_match_x16(feat, other, -1.0, False, True)
            res = [out, stats] + list(_matching.flow_global_match_grad(feat.float(), other.float(), -1.0, stats, g))
            allocations, callers = 5, ["flow_global_match_grad", "flow_global_match_x16"]
        torch.cuda.synchronize()
    finally:
        _matching.torch = torch
    assert harness.callers() == callers
    assert len(harness.log) == allocations
    harness.check_guards()
    harness.check_inputs_unchanged()
    return res


@pytest.mark.parametrize("what", ["forward", "forward-bare", "backward"])
def test_same_bits_under_every_fill(what):
    for n, c, h, w in CASES:
        for name in NAMES:
            _same_bits(n, c, h, w, name, what)


def _same_bits(n, c, h, w, name, what):
    results = [_run(fill, name, n, c, h, w, what) for fill in dm.FILLS]
    for fill, res in zip(dm.FILLS[1:], results[1:]):
        dm.assert_same_bits(res, results[0], "%s under fill 0x%02X against 0x00" % (what, fill))
    _, _, fup, oup = xo.features_general(name, n, c, h, w)                                    # ... and they are the right ones
    want = xo.compute(fup, oup, -1.0)
    got = results[0][0].cpu().numpy()
    assert got.dtype == np.float32 and np.all(np.abs(got - want['out']) <= want['bar'])
    if what == "backward":
        gr = xo.grads(fup, oup, -1.0, mo.upstream(n, h, w), name, want)
        for t, key in ((results[0][2], 'feat'), (results[0][3], 'other')):
            got = t.to(xo.DTYPES[name]).float().cpu().numpy()
            assert np.all(np.abs(got - gr['d_' + key]) <= gr['bar_' + key])
