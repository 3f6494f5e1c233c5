"""Flow.consistency / consistency_mask / filter_consistent on dirty, guarded memory (tests/dirty_memory.py).

`_consistency` allocates its outputs and its workspace with `torch.empty` under its own module-level name `torch`; here that name is a
`dirty_memory.Harness` proxy, so every such tensor is carved out of a buffer  guard | body | guard  whose body holds the fill byte.  For
every combination of optional outputs the public methods ask for: the same bits under the fills 0x00, 0xFF and 0x55 (nothing stale is
read: not the workspace, not an output), bool outputs hold the bytes 0 and 1 only, no guard of any allocation is written, and the
inputs -- guarded copies, their guards holding the fill byte -- are unchanged."""
import numpy as np
import pytest
import torch

import consistency_oracle as co
import dirty_memory as dm

pytestmark = pytest.mark.gpu

FRAMES = [(2, 5, 7), (3, 8, 12), (2, 67, 131)]      # per-element, vector, 9 blocks per image
# (want_error, want_consistent, want_known, want_record): Flow.consistency; Flow.consistency_mask and Flow.filter_consistent
WANTS = {"consistency": (True, True, True, True), "consistency_mask": (False, True, False, False)}


def _run(fill, n, h, w, ref, wants, half):
    from oflibpytorch_amd import _consistency
    dev = torch.device('cuda', 0)
    alpha, beta = co.frame_params(n, h, w)
    a, back, am, bm = (torch.from_numpy(x.copy()).to(dev) for x in co.case(n, h, w, ref))
    if half:
        a, back = a.half(), back.half()
    harness = dm.Harness(fill)
    a, back, am, bm = harness.guard_all(a, back, am, bm)
    assert _consistency.torch is torch
    _consistency.torch = harness.proxy
    try:
        res = _consistency.flow_consistency(a, back, am, bm, -1.0 if ref == 's' else 1.0, alpha, beta, *wants)
        torch.cuda.synchronize()
    finally:
        _consistency.torch = torch
    assert harness.callers() == ["flow_consistency"]
    assert len(harness.log) == sum(wants) + (1 if wants[3] else 0)          # each output wanted, and the workspace with the record
    assert [r is not None for r in res] == list(wants)
    harness.check_guards()
    harness.check_inputs_unchanged()
    dm.assert_bool_bytes(res, "fill 0x%02X" % fill)
    return res


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("method", sorted(WANTS))
@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("n,h,w", FRAMES)
def test_same_bits_under_every_fill(n, h, w, ref, method, half):
    results = [_run(fill, n, h, w, ref, WANTS[method], half) for fill in dm.FILLS]
    for fill, res in zip(dm.FILLS[1:], results[1:]):
        dm.assert_same_bits(res, results[0], "%s under fill 0x%02X against 0x00" % (method, fill))
    if not half:                                                             # ... and they are the right bits
        want = co.reference(n, h, w, ref)
        err, cons, known, rec = results[0]
        assert np.array_equal(cons.cpu().numpy(), want['consistent'])
        if err is not None:
            assert np.array_equal(err.cpu().numpy().view(np.uint32), want['error'].view(np.uint32))
            assert np.array_equal(known.cpu().numpy(), want['known'])
            assert rec[:, :2].tolist() == want['records'][:, :2].tolist() and not bool(rec[:, 5:].any())


@pytest.mark.parametrize("fill", dm.FILLS)
def test_the_public_methods_under_the_proxy(fill):
    """The three methods end to end (filter_consistent included) with every allocation of the binding dirty and guarded."""
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _consistency
    n, h, w, ref = 3, 8, 12, 's'
    dev = torch.device('cuda', 0)
    a, back, am, bm = (torch.from_numpy(x.copy()).to(dev) for x in co.case(n, h, w, ref))
    fa, fb = ofl.Flow(a, ref, am), ofl.Flow(back, ref, bm)
    want = co.reference(n, h, w, ref)
    harness = dm.Harness(fill)
    _consistency.torch = harness.proxy
    try:
        res = fa.consistency(fb, beta=co.TABLE_BETA)
        only = fa.consistency_mask(fb, beta=co.TABLE_BETA)
        filtered = fa.filter_consistent(fb, beta=co.TABLE_BETA)
        torch.cuda.synchronize()
    finally:
        _consistency.torch = torch
    harness.check_guards()
    assert len(harness.log) == 5 + 1 + 1
    dm.assert_bool_bytes([res['consistent'], res['known'], only, filtered.mask], "fill 0x%02X" % fill)
    assert np.array_equal(res['error'].cpu().numpy().view(np.uint32), want['error'].view(np.uint32))
    assert np.array_equal(only.cpu().numpy(), want['consistent']) and np.array_equal(res['known'].cpu().numpy(), want['known'])
    assert np.array_equal(filtered.mask.cpu().numpy(), am.cpu().numpy() & want['consistent'])
    assert res['count'].tolist() == want['records'][:, 0].tolist()
