"""Flow.chain on dirty, guarded memory (tests/dirty_memory.py).

`_chain` allocates its two outputs with `torch.empty` under its own module-level name `torch`; here that name is a `dirty_memory.Harness`
proxy, so both tensors are carved out of a buffer  guard | body | guard  whose body holds the fill byte.  With and without `return_all`:
the same bits under the fills 0x00, 0xFF and 0x55, which are the oracle's (every element of both outputs is written, vectors under a
false mask included, and nothing stale is read), the mask holds the bytes 0 and 1 only, no guard of either allocation is written, and the
inputs -- guarded copies, their guards holding the fill byte -- are unchanged."""
import numpy as np
import pytest
import torch

import chain_oracle as co
import dirty_memory as dm

pytestmark = pytest.mark.gpu

CASES = [(1, 2, 2, 2), (2, 5, 7, 3), (2, 20, 28, 5), (2, 67, 131, 3)]      # (n, h, w, T): one lane in four, odd sizes, 35 blocks with a tail


def _run(fill, n, h, w, t, ref, want_all, half):
    from oflibpytorch_amd import _chain
    dev = torch.device('cuda', 0)
    flows, masks = co.case(n, h, w, ref, t)
    vs = [torch.from_numpy(np.array(f)).to(dev) for f in flows]
    if half:
        vs = [v.half() if k % 2 else v for k, v in enumerate(vs)]
    ms = [None if m is None else torch.from_numpy(np.array(m)).to(dev) for m in masks]
    harness = dm.Harness(fill)
    vs, ms = list(harness.guard_all(*vs)), list(harness.guard_all(*ms))
    assert _chain.torch is torch
    _chain.torch = harness.proxy
    try:
        res = _chain.flow_chain(vs, ms, -1.0 if ref == 's' else 1.0, want_all)
        torch.cuda.synchronize()
    finally:
        _chain.torch = torch
    assert harness.callers() == ["flow_chain"] and len(harness.log) == 2            # the vectors and the mask, nothing else
    lead = (t - 1,) if want_all else ()
    assert tuple(res[0].shape) == lead + (n, 2, h, w) and tuple(res[1].shape) == lead + (n, h, w)
    harness.check_guards()
    harness.check_inputs_unchanged()
    dm.assert_bool_bytes(res, "fill 0x%02X" % fill)
    return res


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("want_all", [False, True], ids=["chain", "all"])
@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("n,h,w,t", CASES)
def test_same_bits_under_every_fill(n, h, w, t, ref, want_all, half):
    results = [_run(fill, n, h, w, t, ref, want_all, half) for fill in dm.FILLS]
    for fill, res in zip(dm.FILLS[1:], results[1:]):
        dm.assert_same_bits(res, results[0], "fill 0x%02X against 0x00" % fill)
    if not half:                                                                   # ... and they are the right bits
        vecs, valid, _ = co.reference(n, h, w, ref, t)
        ks = (range(1, t) if ref == 's' else range(0, t - 1)) if want_all else [t - 1 if ref == 's' else 0]
        want_v, want_m = np.stack([vecs[k] for k in ks]), np.stack([valid[k] for k in ks])
        got_v, got_m = results[0][0].cpu().numpy(), results[0][1].cpu().numpy()
        if not want_all:
            got_v, got_m = got_v[None], got_m[None]
        assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32)) and np.array_equal(got_m, want_m)


@pytest.mark.parametrize("fill", dm.FILLS)
def test_the_public_method_under_the_proxy(fill):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _chain
    n, h, w, t, ref = 2, 20, 28, 5, 't'
    dev = torch.device('cuda', 0)
    flows, masks = co.case(n, h, w, ref, t)
    objs = [ofl.Flow(torch.from_numpy(np.array(f)).to(dev), ref, None if m is None else torch.from_numpy(np.array(m)).to(dev))
            for f, m in zip(flows, masks)]
    vecs, valid, _ = co.reference(n, h, w, ref, t)
    harness = dm.Harness(fill)
    _chain.torch = harness.proxy
    try:
        one = ofl.Flow.chain(objs)
        every = ofl.Flow.chain(objs, return_all=True)
        torch.cuda.synchronize()
    finally:
        _chain.torch = torch
    harness.check_guards()
    assert len(harness.log) == 4
    dm.assert_bool_bytes([one.mask] + [e.mask for e in every], "fill 0x%02X" % fill)
    assert np.array_equal(one.vecs.cpu().numpy().view(np.uint32), vecs[0].view(np.uint32)) and np.array_equal(one.mask.cpu().numpy(), valid[0])
    for k in range(t):
        assert np.array_equal(every[k].vecs.cpu().numpy().view(np.uint32), vecs[k].view(np.uint32)), k
        assert np.array_equal(every[k].mask.cpu().numpy(), valid[k]), k
