"""CPU tier of Flow.chain / chain_flows: the oracle (tests/chain_oracle.py) against the fold of
`Flow.combine_with(..., 3)` on the C oracle, which the reference's fixtures pin; the conditions on the inputs the GPU tier runs on and the
pixels planted in them; the host logic of the API with the native call served by the oracle; the C ABI's declarations and argument
checks.  No device."""
import ctypes

import numpy as np
import pytest
import torch

import chain_oracle as co

# (h, w, T) of the table the GPU tier runs as well: T = 32 at 20 x 28 only
TABLE = [(h, w, t) for h, w in co.FRAMES for t in (2, 3, 5)] + [(20, 28, 32)]
BIG = [c for c in TABLE if c[0] >= 20]


@pytest.fixture
def chain_native(oracle_native, monkeypatch):
    from oflibpytorch_amd import _chain
    monkeypatch.setattr(_chain, "flow_chain", co.fake_flow_chain)
    return _chain


def _flows(flows, masks, ref):
    from oflibpytorch_amd import Flow
    return [Flow(torch.from_numpy(f.copy()), ref, None if m is None else torch.from_numpy(m.copy())) for f, m in zip(flows, masks)]


_fold = co.fold


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ---- the oracle is the fold, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("h,w,t", TABLE)
def test_oracle_is_the_fold_of_mode_3_bit_for_bit(oracle_native, h, w, t, n, ref):
    flows, masks = co.case(n, h, w, ref, t)
    vecs, valid, _ = co.reference(n, h, w, ref, t)
    fold = _fold(_flows(flows, masks, ref), ref)
    assert len(fold) == len(vecs) == t
    for k in range(t):                                        # every prefix ('s') / suffix ('t') of return_all
        assert _same_bits(vecs[k], fold[k].vecs.numpy()), (k, "vectors")
        assert np.array_equal(valid[k], fold[k].mask.numpy()), (k, "mask")


def test_oracle_on_cases_written_out_by_hand():
    """Integer translations: f_1 = (2, 1), f_2 = (1, 0), f_3 = (0, 1) on a 5 x 6 frame; the chain is (3, 2) wherever the walk stays
    inside, and the walk's own samples turn to 0 where it has left (the vectors are still the sum of what it read)."""
    h, w = 5, 6
    fl = [np.zeros((1, 2, h, w), np.float32) for _ in range(3)]
    fl[0][:, 0], fl[0][:, 1] = 2, 1
    fl[1][:, 0] = 1
    fl[2][:, 1] = 1
    vecs, valid = co.chain(fl, [None] * 3, 's')
    want = np.zeros((h, w), bool)
    want[:h - 1, :w - 3] = True                                # f_3 is read at p + (3, 1): the mask speaks of the samples, not of the end point
    assert np.array_equal(valid[2][0], want)
    assert (vecs[2][0, 0][want] == 3).all() and (vecs[2][0, 1][want] == 2).all()
    assert vecs[2][0, 0, 0, w - 1] == 2 and vecs[2][0, 1, 0, w - 1] == 1          # left at the first step: reads 0 from then on
    assert np.array_equal(valid[1][0], np.pad(np.ones((h - 1, w - 2), bool), ((0, 1), (0, 2))))     # f_2 is read at p + (2, 1)
    # 't': the walk runs backward in time, positions x - acc
    vecs, valid = co.chain(fl, [None] * 3, 't')
    want = np.zeros((h, w), bool)
    want[1:, 1:] = True                                        # f_2 is read at x - (0, 1), f_1 at x - (1, 1)
    assert np.array_equal(valid[0][0], want) and (vecs[0][0, 0][want] == 3).all() and (vecs[0][0, 1][want] == 2).all()
    assert _same_bits(vecs[2], fl[2]) and valid[2].all()
    # a mask hole at the landing point of one pixel invalidates that pixel alone; its vectors are what they were
    m2 = np.ones((1, h, w), bool)
    m2[0, 2, 3] = False                                        # f_2 is read at p + (2, 1): pixel (1, 1)
    v2, k2 = co.chain(fl, [None, m2, None], 's')
    want = np.zeros((h, w), bool)
    want[:h - 1, :w - 3] = True
    want[1, 1] = False
    assert np.array_equal(k2[2][0], want) and _same_bits(v2[2], co.chain(fl, [None] * 3, 's')[0][2])


# ---- the inputs of the GPU tier ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("h,w,t", BIG)
def test_the_inputs_meet_their_conditions(h, w, t, n, ref):
    """Conditions on the inputs, not tolerances: in every frame of 20 x 28 and more at least 25 % of the pixels are valid in the final
    mask and at least 5 % have been invalidated by the walk itself, not by the mask of the flow the walk starts from."""
    flows, masks = co.case(n, h, w, ref, t)
    _, valid, _ = co.reference(n, h, w, ref, t)
    order = co.walk_order(t, ref)
    start, final = valid[order[0]], valid[order[-1]]
    shares = {'valid': final.mean(), 'by_the_walk': (start & ~final).mean()}
    print(shares)
    assert shares['valid'] >= 0.25 and shares['by_the_walk'] >= 0.05, shares
    assert masks[co.none_mask_index(t, ref)] is None and sum(m is None for m in masks) == 1
    for m in masks:
        if m is not None:
            assert 0.08 < 1.0 - m.mean() < 0.25                # about 15 % holes


@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("t", [2, 3, 5, 32])
def test_the_planted_pixels_hit_what_they_name(t, n, ref):
    h, w = co.PLANT_FRAME
    flows, masks = co.case(n, h, w, ref, t)
    vecs, valid, det = co.reference(n, h, w, ref, t)
    order = co.walk_order(t, ref)
    final_v, final_m = vecs[order[-1]], valid[order[-1]]
    d2 = det[0]                                               # the step that reads the walk's second flow ("step 2")
    wts = lambda d, y, x: [float(wt[i, y, x]) for wt in d['weights']]
    for i in range(n):
        # (a) outside the frame at step 2, inside at step 3; the mask is false, the vectors go on being accumulated
        y, x = co.PLANTED['a']
        assert w - 1 < d2['sx'][i, y, x] < w and not d2['inside'][1][i, y, x] and d2['mr'][i, y, x] < co.VALID_THRESHOLD
        assert not valid[order[1]][i, y, x] and not final_m[i, y, x]
        if t >= 3:
            d3 = det[1]
            assert 0 <= d3['sx'][i, y, x] <= w - 1 and 0 <= d3['sy'][i, y, x] <= h - 1 and all(k[i, y, x] for k in d3['inside'])
            assert abs(d3['sx'][i, y, x] - 23.5) < 0.01
            before, after = vecs[order[1]][i, :, y, x], vecs[order[2]][i, :, y, x]
            assert (before != after).any()                      # still accumulated under a false mask, back inside the frame
        # (b) integer positions: weights 1, 0, 0, 0
        y, x = co.PLANTED['b']
        assert (d2['sx'][i, y, x], d2['sy'][i, y, x]) == (8.0, 9.0) and wts(d2, y, x) == [1.0, 0.0, 0.0, 0.0]
        assert tuple(np.abs(vecs[order[1]][i, :, y, x])) == (abs(11.0 - x), abs(7.0 - y))
        for d in det[1:]:
            assert (d['sx'][i, y, x], d['sy'][i, y, x]) == (11.0, 7.0) and wts(d, y, x) == [1.0, 0.0, 0.0, 0.0]
        assert final_m[i, y, x]
        # (c) the last column and row: east and south taps outside at weight 0, mr = 1, valid
        y, x = co.PLANTED['c']
        for d in det:
            assert (d['sx'][i, y, x], d['sy'][i, y, x]) == (w - 1.0, h - 1.0) and wts(d, y, x) == [1.0, 0.0, 0.0, 0.0]
            assert [bool(k[i, y, x]) for k in d['inside']] == [True, False, False, False] and d['mr'][i, y, x] == 1.0
        assert final_m[i, y, x]
        # (d) a tap in a mask hole at weight exactly 0: still valid
        y, x = co.PLANTED['d']
        assert wts(d2, y, x) == [1.0, 0.0, 0.0, 0.0] and d2['inside'][1][i, y, x] and not d2['valid'][1][i, y, x]
        assert d2['mr'][i, y, x] == 1.0 and valid[order[1]][i, y, x] and final_m[i, y, x]
        # (e) a tap in a mask hole at weight > 0: invalid from that step on, in every later prefix
        y, x = co.PLANTED['e']
        assert 0.4 < wts(d2, y, x)[1] < 0.6 and d2['inside'][1][i, y, x] and not d2['valid'][1][i, y, x] and 0.4 < d2['mr'][i, y, x] < 0.6
        assert valid[order[0]][i, y, x] and not any(valid[k][i, y, x] for k in order[1:])
    assert np.isfinite(final_v).all()


def test_the_input_recipe():
    flows, masks = co.case(2, 67, 131, 's', 5)
    assert co.case(2, 67, 131, 's', 5)[0] is flows and not flows[0].flags.writeable           # computed once, shared, read-only
    assert all(f.dtype == np.float32 and f.shape == (2, 2, 67, 131) for f in flows)
    assert all(m is None or (m.dtype == bool and m.shape == (2, 67, 131)) for m in masks)
    assert not np.array_equal(flows[0], flows[1]) and not np.array_equal(flows[0][0], flows[0][1])
    total = np.sum([f.astype(np.float64) for f in flows], 0)
    assert 1.0 < np.abs(total).max() < 8.0                                                     # a few pixels whatever T is
    assert co.reference(2, 67, 131, 's', 5) is co.reference(2, 67, 131, 's', 5)


# ---- the API, with the native call served by the oracle ---------------------------------------------------------------------------------
def _objs(n=2, h=5, w=7, ref='s', t=3):
    return _flows(*co.case(n, h, w, ref, t), ref)


def test_argument_checks_messages_and_order(chain_native):
    from oflibpytorch_amd import Flow
    a, b, c = _objs()
    other_shape = _objs(h=8, w=12)[0]
    other_batch = _objs(n=1)[0]
    other_ref = _objs(ref='t')[0]
    thin = Flow(torch.zeros(2, 2, 1, 7), 's')
    cases = [
        (TypeError, "Flows needs to be a list or a tuple of flow objects", (a,), {}),                       # (a Flow, not a list)
        (TypeError, "Flows needs to be a list or a tuple of flow objects", ([a, a.vecs],), {}),
        (ValueError, "The sequence needs to hold 1 to 32 flows", ([],), {}),
        (ValueError, "The sequence needs to hold 1 to 32 flows", ([a] * 33,), {}),
        (ValueError, "Flow fields need to have the same shape, including batch size", ([a, other_shape],), {}),
        (ValueError, "Flow fields need to have the same shape, including batch size", ([a, other_batch],), {}),
        (ValueError, "Flow fields need to have the same reference: switch_ref the others", ([a, other_ref],), {}),
        (ValueError, "Flow fields need to be at least 2 pixels high and wide", ([thin, thin],), {}),
        (TypeError, "Return_all needs to be boolean", ([a, b],), {'return_all': 1}),
    ]
    for exc, msg, args, kw in cases:
        with pytest.raises(exc) as info:
            Flow.chain(args[0], **kw)
        assert str(info.value) == "Error chaining flows: " + msg
    # the order: the type of the list before its length, the length before the shapes, the shapes before the references, the references
    # before the size, the size before return_all
    with pytest.raises(TypeError, match="list or a tuple"):
        Flow.chain([a.vecs] * 40, return_all=1)
    with pytest.raises(ValueError, match="1 to 32"):
        Flow.chain([a] * 32 + [other_shape], return_all=1)
    with pytest.raises(ValueError, match="same shape"):
        Flow.chain([a, Flow(torch.zeros(2, 2, 5, 7), 't'), other_shape], return_all=1)
    with pytest.raises(ValueError, match="same reference"):
        Flow.chain([thin, Flow(torch.zeros(2, 2, 1, 7), 't')], return_all=1)
    with pytest.raises(ValueError, match="at least 2 pixels"):
        Flow.chain([thin, thin], return_all=1)


def test_a_single_flow_is_returned_as_it_is(chain_native, monkeypatch):
    from oflibpytorch_amd import Flow
    monkeypatch.setattr(chain_native, "flow_chain", None)    # no launch: calling it would raise
    a = _objs()[0]
    assert Flow.chain([a]) is a and Flow.chain((a,), return_all=False) is a
    out = Flow.chain([a], return_all=True)
    assert isinstance(out, list) and len(out) == 1 and out[0] is a


@pytest.mark.parametrize("ref", ['s', 't'])
def test_return_all_layout_and_result(chain_native, ref):
    from oflibpytorch_amd import Flow
    n, h, w, t = 2, 8, 12, 5
    objs = _objs(n, h, w, ref, t)
    vecs, valid, _ = co.reference(n, h, w, ref, t)
    full = t - 1 if ref == 's' else 0
    single = 0 if ref == 's' else t - 1
    res = Flow.chain(objs)
    assert isinstance(res, Flow) and res.ref == ref and res.shape == objs[0].shape and res.vecs.dtype == torch.float32
    assert _same_bits(res.vecs.numpy(), vecs[full]) and np.array_equal(res.mask.numpy(), valid[full])
    out = Flow.chain(tuple(objs), return_all=True)
    assert isinstance(out, list) and len(out) == t and out[single] is objs[single]
    for k in range(t):
        assert out[k].ref == ref and _same_bits(out[k].vecs.numpy(), vecs[k]) and np.array_equal(out[k].mask.numpy(), valid[k]), k
    parts = [o for k, o in enumerate(out) if k != single]
    base = parts[0]._vecs.untyped_storage().data_ptr()
    mbase = parts[0]._mask.untyped_storage().data_ptr()
    assert all(o._vecs.untyped_storage().data_ptr() == base and o._mask.untyped_storage().data_ptr() == mbase for o in parts)   # one allocation each
    # the fold gives the same flows (no early exit on these inputs)
    fold = _fold(objs, ref)
    for k in range(t):
        assert _same_bits(out[k].vecs.numpy(), fold[k].vecs.numpy()) and np.array_equal(out[k].mask.numpy(), fold[k].mask.numpy())


def test_what_the_native_call_receives(oracle_native, monkeypatch):
    """The vectors as stored and detached, the masks as they are (None included), the sign of the reference, return_all."""
    from oflibpytorch_amd import Flow, _chain
    seen = []

    def spy(vecs, masks, flow_sign=-1.0, want_all=False):
        seen.append((vecs, masks, flow_sign, want_all))
        return co.fake_flow_chain(vecs, masks, flow_sign, want_all)

    monkeypatch.setattr(_chain, "flow_chain", spy)
    for ref, sign in (('s', -1.0), ('t', 1.0)):
        objs = _objs(ref=ref)
        Flow.chain(objs, return_all=(ref == 't'))
        vecs, masks, flow_sign, want_all = seen[-1]
        assert flow_sign == sign and want_all is (ref == 't') and len(vecs) == len(masks) == 3
        assert all(v.data_ptr() == o._fv.data_ptr() and not v.requires_grad for v, o in zip(vecs, objs))
        assert [m is None for m in masks] == [o._mask is None for o in objs] and sum(m is None for m in masks) == 1


def test_requires_grad_takes_the_fold(oracle_native, monkeypatch):
    """With autograd recording and a flow whose vectors require a gradient the call runs the fold of combine_with; the fused call is not
    made.  (The oracle-backed primitives of this tier are forward-only, so the fold is replaced by a recorder.)"""
    from oflibpytorch_amd import Flow, _chain
    monkeypatch.setattr(_chain, "flow_chain", None)
    calls = []
    monkeypatch.setattr(Flow, "_chain_fold", staticmethod(lambda flows, return_all: calls.append((flows, return_all)) or "folded"))
    objs = _objs()
    objs[1]._vecs.requires_grad_(True)
    assert Flow.chain(objs, return_all=True) == "folded" and calls[-1][1] is True and [f for f in calls[-1][0]] == objs
    with torch.no_grad():
        monkeypatch.setattr(_chain, "flow_chain", co.fake_flow_chain)
        assert isinstance(Flow.chain(objs), Flow) and len(calls) == 1


@pytest.mark.parametrize("ref", ['s', 't'])
def test_chain_fold_is_the_explicit_fold(oracle_native, ref):
    from oflibpytorch_amd import Flow
    objs = _objs(2, 8, 12, ref, 3)
    want = _fold(objs, ref)
    got = Flow._chain_fold(objs, True)
    assert len(got) == 3
    for g, w_ in zip(got, want):
        assert _same_bits(g.vecs.numpy(), w_.vecs.numpy()) and np.array_equal(g.mask.numpy(), w_.mask.numpy())
    one = Flow._chain_fold(objs, False)
    full = want[-1] if ref == 's' else want[0]
    assert _same_bits(one.vecs.numpy(), full.vecs.numpy())


def test_the_adapter(chain_native):
    import oflibpytorch_amd as ofl
    n, h, w, t = 2, 8, 12, 3
    flows, masks = co.case(n, h, w, 's', t)
    vecs, valid, _ = co.reference(n, h, w, 's', t)
    out = ofl.chain_flows([torch.from_numpy(f.copy()) for f in flows], 's')
    assert isinstance(out, torch.Tensor) and tuple(out.shape) == (n, 2, h, w)
    no_masks = co.chain(flows, [None] * t, 's')
    assert _same_bits(out.numpy(), no_masks[0][-1])
    v, m = ofl.chain_flows([f.copy() for f in flows], 's', masks=[None if k is None else k.copy() for k in masks])    # ndarrays
    assert _same_bits(v.numpy(), vecs[-1]) and np.array_equal(m.numpy(), valid[-1]) and m.dtype == torch.bool
    # 3-D in, 3-D out
    v3, m3 = ofl.chain_flows([f[0].copy() for f in flows], 's', masks=[None if k is None else k[0].copy() for k in masks])
    assert tuple(v3.shape) == (2, h, w) and tuple(m3.shape) == (h, w)
    assert _same_bits(v3.numpy(), vecs[-1][0]) and np.array_equal(m3.numpy(), valid[-1][0])
    every = ofl.chain_flows([f[0].copy() for f in flows], 's', return_all=True)
    assert isinstance(every, list) and len(every) == t and all(tuple(e.shape) == (2, h, w) for e in every)
    assert _same_bits(every[1].numpy(), no_masks[0][1][0])
    pairs = ofl.chain_flows(list(flows), 's', masks=list(masks), return_all=True)
    assert all(isinstance(p, tuple) and tuple(p[0].shape) == (n, 2, h, w) and tuple(p[1].shape) == (n, h, w) for p in pairs)
    for bad, exc in (((flows[0], 's'), TypeError), (([1, 2], 's'), TypeError), (([], 's'), ValueError)):
        with pytest.raises(exc, match="Error chaining flows: "):
            ofl.chain_flows(*bad)
    with pytest.raises(TypeError, match="Error chaining flows: Masks"):
        ofl.chain_flows(list(flows), 's', masks=[None])
    with pytest.raises(ValueError):
        ofl.chain_flows(list(flows), 'x')


# ---- the C ABI: declared, exported, and every rejected argument is rejected before any launch -----------------------------------------
def test_c_abi_declarations_and_argument_checks_need_no_gpu():
    from oflibpytorch_amd import _chain, _native
    assert "ofl_flow_chain_f32" in set(_native.exported_symbols())
    header = open(_native._build.HEADERS[0]).read()
    assert " ofl_flow_chain_f32(" in header and "#define OFL_CHAIN_MAX_T %d\n" % _chain.MAX_T in header
    assert any(src.endswith("ofl_chain.hip") for src in _native._build.SOURCES)
    lib = _chain._library()
    assert hasattr(lib, "ofl_flow_chain_f32")                           # present in the built library
    assert lib.ofl_version() == _native.ABI_VERSION == 36                # a name was added, no signature changed
    assert lib.ofl_flow_chain_f32.argtypes[5] is ctypes.c_int32 and lib.ofl_flow_chain_f32.argtypes[6] is ctypes.c_float
    for what, kw in co.rejected_calls():
        assert co.call_abi(lib, **kw) == -3, what                        # OFL_E_ARG
