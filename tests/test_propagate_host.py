"""CPU tier of Flow.propagate: the oracle (tests/propagate_oracle.py) against the two textbook expressions in torch
float64 -- softmax(Q K^T / sqrt(C)) flow, and GMFlow's unfold with zero padding -- and their autograd, six mutants that the comparison
must tell apart, the exact-softmax inputs of the GPU tier, the host logic of the API with the native calls served by the oracle, every
argument check that needs no device, and the C ABI's declarations and argument checks.  No device."""
import ctypes

import numpy as np
import pytest
import torch

import propagate_oracle as po

SHAPES = ((5, 7), (9, 11))
RADII = (None, 1, 2, 3, 4)
N = 2


@pytest.fixture
def pp_native(oracle_native, monkeypatch):
    from oflibpytorch_amd import _propagate
    monkeypatch.setattr(_propagate, "flow_propagate", po.fake_flow_propagate)
    monkeypatch.setattr(_propagate, "flow_propagate_grad", po.fake_flow_propagate_grad)
    return _propagate


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x).copy())


def _mask(n, h, w):
    """about a third of the positions excluded; never a whole image or, for the smallest window, a whole interior window"""
    m = np.random.RandomState(17 + h + w).uniform(size=(n, h, w)) > 0.3
    assert m.any((1, 2)).all() and not m.all()
    return m


# ---- the oracle computes the textbook expressions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("c", [1, 5, 16])
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("h,w", SHAPES)
def test_float64_evaluation_is_the_textbook_expression_and_its_autograd(h, w, radius, c, masked):
    """A batch of 2: the oracle's float64 evaluation (float64 logits; the streaming chain with its rescales, or the two passes over the
    window with its padded positions at logit 0 and vector 0) and its three gradients against the torch float64 expression and torch's
    autograd of it, within 1e-12 of each result's scale.  Excluded positions are at -inf in the textbook."""
    query, key = po.features_general(N, c, h, w)
    flow, g = po.vectors(N, h, w), po.upstream(N, h, w)
    mask = _mask(N, h, w) if masked else None
    want = po.textbook(flow, mask, query, key, radius, g)
    assert np.isfinite(want['out']).all()
    got = po.compute(flow, mask, query, key, radius, wide=True)
    gr = po.grads(flow, mask, query, key, radius, g, wide=True)
    assert got['valid'].all()
    for name, a, b in (("out", got['out'], want['out']), ("d query", gr['d_query'], want['d_query']),
                       ("d key", gr['d_key'], want['d_key']), ("d flow", gr['d_flow'], want['d_flow'])):
        scale = np.abs(b).max()
        err = np.abs(a - b).max()
        print("%d x %d r %s C %d %s: largest |oracle float64 - textbook float64| = %.3e of a scale %.3e" % (h, w, radius, c, name, err, scale))
        assert a.dtype == np.float64 and a.shape == b.shape and scale > 0
        assert err <= 1e-12 * scale, name
    # the definition's float32 results are the float32-logit evaluation rounded once, and close to the textbook's
    d = po.compute(flow, mask, query, key, radius)
    assert np.array_equal(d['out32'], d['out'].astype(np.float32))
    assert np.abs(d['out'] - want['out']).max() <= 1e-4 * np.abs(want['out']).max()


def test_the_issue_s_check_of_the_local_definition():
    """4 x 6, C = 5, r = 2: the definition equals softmax((q . unfold(k)).sum(C) / sqrt(C)) . unfold(flow) with padding r, forward and
    all three gradients, within 1e-12 (measured: a few 1e-16)"""
    n, c, h, w, r = 1, 5, 4, 6, 2
    query, key = po.features_general(n, c, h, w)
    flow, g = po.vectors(n, h, w), po.upstream(n, h, w)
    want = po.textbook(flow, None, query, key, r, g)
    got, gr = po.compute(flow, None, query, key, r, wide=True), po.grads(flow, None, query, key, r, g, wide=True)
    for a, b in ((got['out'], want['out']), (gr['d_query'], want['d_query']), (gr['d_key'], want['d_key']), (gr['d_flow'], want['d_flow'])):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


@pytest.mark.parametrize("mutant", po.MUTANTS)
def test_mutants_fail_the_comparison(mutant):
    """The softmax over p instead of q, the 1 / sqrt(C) dropped, u and v swapped, padded positions excluded instead of zero, masked
    positions not excluded and the values of a window taken dx-outermost each compute another function: each must miss by more than a
    tenth of the result's scale, on inputs where the oracle itself is within 1e-12"""
    h, w, c = 5, 7, 5
    radius = None if mutant == "over_p" else 2
    query, key = po.features_general(N, c, h, w)
    flow = po.vectors(N, h, w)
    mask = _mask(N, h, w)
    want = po.textbook(flow, mask, query, key, radius)['out']
    scale = np.abs(want).max()
    miss = np.abs(po.compute(flow, mask, query, key, radius, wide=True, mutant=mutant)['out'] - want).max()
    print("%s: misses by %.3f of the scale" % (mutant, miss / scale))
    assert miss > 0.1 * scale
    assert np.abs(po.compute(flow, mask, query, key, radius, wide=True)['out'] - want).max() <= 1e-12 * scale


@pytest.mark.parametrize("radius", [None, 1, 4])
@pytest.mark.parametrize("c", [4, 16])
def test_the_exact_inputs_are_what_they_say(c, radius):
    """The bit-for-bit tier of the GPU tests rests on these: every logit, and the padded +0, is 0 or at most -1024 and so is every
    difference of two, so every exp is 1 or +0; the padded logit ties with the maximum; the vectors sit on a grid of 2^-6, so the
    float64 sums are exact and S is a whole number"""
    n, h, w = 3, 5, 13
    flow = po.vectors(n, h, w)
    assert np.array_equal(flow * 64, np.round(flow * 64)) and np.abs(flow).max() <= 4
    tied = 0
    for kind in po.exact_kinds(c):
        query, key = po.features_exact(kind, n, c, h, w)
        for name, mask in po.masks(n, h, w, radius).items():
            r = po.compute(flow, mask, query, key, radius)
            s = r['s']
            assert ((s == 0) | (s <= -1024)).all(), kind
            live = r['valid'].reshape(n, -1)
            e = r['w'] * r['S'][:, :, None]
            assert np.isin(e[live], (0.0, 1.0)).all() and np.array_equal(r['S'], np.round(r['S'])), (kind, name)
            assert (r['S'][live] >= 1).all() and (r['S'][~live] == 0).all() and (r['out32'].reshape(n, 2, -1).transpose(0, 2, 1)[~live] == 0).all()
            if radius is not None:
                pad = ~r['inside'][None] & (r['m'][:, :, None] == 0) & ((s == 0) & r['inside'][None] & r['part']).any(2, keepdims=True)
                tied += int(pad.sum())
            if name == 'one-image-masked':
                assert not r['valid'][n - 1].any() and r['valid'][:n - 1].all()
            if name == 'block' and radius == 1:
                assert not r['valid'][:, 1:4, 1:4].any()                                       # empty pixels inside the masked block
    assert radius is None or tied > 0                                                        # the padded +0 ties with a match's logit


def test_an_excluded_position_changes_no_bit_of_the_forward():
    n, c, h, w = 1, 3, 4, 5
    query, key = (a.copy() for a in po.features_general(n, c, h, w))
    flow = po.vectors(n, h, w).copy()
    mask = np.ones((n, h, w), bool)
    mask[0, 2, 3] = False
    for radius in (None, 2):
        clean = po.compute(flow, mask, query, key, radius)
        k2, f2 = key.copy(), flow.copy()
        k2[0, :, 2, 3] = np.nan
        f2[0, :, 2, 3] = np.nan
        dirty = po.compute(f2, mask, query, k2, radius)
        assert np.array_equal(clean['out32'].view(np.uint32), dirty['out32'].view(np.uint32))
        assert np.isnan(po.compute(f2, None, query, k2, radius)['out32']).any()


# ---- the host logic of the API, the oracle in the bindings' place ---------------------------------------------------------------------
@pytest.mark.parametrize("radius", [None, 2])
def test_shapes_values_ref_and_result_mask(pp_native, radius):
    import oflibpytorch_amd as ofl
    (h, w), c = SHAPES[0], 5
    query, key = po.features_general(N, c, h, w)
    vec = po.vectors(N, h, w)
    mask = _mask(N, h, w)
    mask[1] = False                                                                          # image 1: every pixel is empty
    want = po.compute(vec, mask, query, key, radius)
    for ref in ('s', 't'):
        flow = ofl.Flow(_t(vec), ref, _t(mask))
        res = flow.propagate(_t(query), _t(key), radius)
        assert isinstance(res, ofl.Flow) and res.ref == ref and res.shape == (N, h, w) and res.device == flow.device
        assert res.vecs.dtype == torch.float32 and not res.vecs.requires_grad
        assert np.array_equal(res.vecs.numpy(), want['out32']) and np.array_equal(res.mask.numpy(), want['valid'])
        assert bool(res.mask[0].all()) and not bool(res.mask[1].any()) and bool((res.vecs[1] == 0).all())
    flow = ofl.Flow(_t(vec), 't', _t(mask))
    free = po.compute(vec, None, query, key, radius)
    res = flow.propagate(_t(query), _t(key), radius, consider_mask=False)
    assert np.array_equal(res.vecs.numpy(), free['out32']) and bool(res.mask.all())
    # key=None is the query itself; arrays are taken; a C-H-W operand serves the whole batch
    same = po.compute(vec, mask, query, query, radius)
    assert np.array_equal(flow.propagate(_t(query), radius=radius).vecs.numpy(), same['out32'])
    assert np.array_equal(flow.propagate(query.copy(), key.copy(), radius).vecs.numpy(), want['out32'])
    one = po.compute(vec, mask, query[:1], key[:1], radius)
    assert np.array_equal(flow.propagate(_t(query[0]), _t(key[0]), radius).vecs.numpy(), one['out32'])
    # the wrapper: vectors, and with a mask the pair
    got = ofl.propagate_flow(_t(vec), _t(query), _t(key), radius)
    assert isinstance(got, torch.Tensor) and got.shape == (N, 2, h, w) and np.array_equal(got.numpy(), free['out32'])
    got, valid = ofl.propagate_flow(_t(vec), _t(query), _t(key), radius, mask=_t(mask))
    assert np.array_equal(got.numpy(), want['out32']) and valid.dtype == torch.bool and np.array_equal(valid.numpy(), want['valid'])
    got, valid = ofl.propagate_flow(_t(vec[0]), _t(query[0]), None, radius, mask=_t(mask[0]))
    assert got.shape == (2, h, w) and valid.shape == (h, w)
    assert np.array_equal(got.numpy(), po.compute(vec[:1], mask[:1], query[:1], query[:1], radius)['out32'][0])
    assert np.array_equal(ofl.propagate_flow(vec[0].copy(), query[0].copy(), radius=radius).numpy(), po.compute(vec[:1], None, query[:1], query[:1], radius)['out32'][0])


@pytest.mark.parametrize("need", ["none", "query", "key", "flow", "all"])
def test_requires_grad_routing(pp_native, monkeypatch, need):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _autograd
    h, w, c, radius = 5, 7, 5, 1
    query, key = po.features_general(N, c, h, w)
    vec, g, mask = po.vectors(N, h, w), po.upstream(N, h, w), _mask(N, h, w)
    calls = []
    real = po.fake_flow_propagate_grad

    def spy(vecs, mask, query, key, radius, stats, grad_out, want_query=True, want_key=True, want_flow=True):
        calls.append((want_query, want_key, want_flow))
        return real(vecs, mask, query, key, radius, stats, grad_out, want_query, want_key, want_flow)
    monkeypatch.setattr(pp_native, "flow_propagate_grad", spy)
    wants = {k: need in (k, "all") for k in ("query", "key", "flow")}
    qt, kt, vt = _t(query).requires_grad_(wants["query"]), _t(key).requires_grad_(wants["key"]), _t(vec).requires_grad_(wants["flow"])
    res = ofl.Flow(vt, 't', _t(mask)).propagate(qt, kt, radius)
    assert issubclass(_autograd.PropagateFn, torch.autograd.Function)
    assert not res.mask.requires_grad
    if need == "none":
        assert not res.vecs.requires_grad and res.vecs.grad_fn is None
        return
    assert res.vecs.requires_grad and type(res.vecs.grad_fn).__name__ == "PropagateFnBackward"
    res.vecs.backward(_t(g))
    assert calls == [(wants["query"], wants["key"], wants["flow"])]
    want = po.grads(vec, mask, query, key, radius, g)
    for t, name in ((qt, 'query'), (kt, 'key'), (vt, 'flow')):
        if wants[name]:
            assert t.grad.dtype == torch.float32 and np.array_equal(t.grad.numpy(), want['d_' + name])
        else:
            assert t.grad is None
    with torch.no_grad():
        assert not ofl.Flow(vt, 't', _t(mask)).propagate(qt, kt, radius).vecs.requires_grad
    if need != "all":
        return
    # key=None: the tensor is passed twice and autograd adds the two gradients
    q2 = _t(query).requires_grad_(True)
    ofl.Flow(_t(vec), 't', _t(mask)).propagate(q2, None, radius).vecs.backward(_t(g))
    both = po.grads(vec, mask, query, query, radius, g)
    assert np.array_equal(q2.grad.numpy(), both['d_query'] + both['d_key'])
    # a C-H-W operand gets a C-H-W gradient: the batch's gradients summed
    q3, k3 = _t(query[0]).requires_grad_(True), _t(key[0]).requires_grad_(True)
    ofl.Flow(_t(vec), 't', _t(mask)).propagate(q3, k3, radius).vecs.backward(_t(g))
    w3 = po.grads(vec, mask, query[:1], key[:1], radius, g)
    assert q3.grad.shape == q3.shape and k3.grad.shape == k3.shape
    assert np.array_equal(q3.grad.numpy(), w3['d_query'].sum(0)) and np.array_equal(k3.grad.numpy(), w3['d_key'].sum(0))


def test_api_checks_and_their_messages(oracle_native, monkeypatch):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _propagate

    def never(*args, **kw):
        raise AssertionError("the checks come before the kernel")
    monkeypatch.setattr(_propagate, "flow_propagate", never)
    monkeypatch.setattr(_propagate, "propagate", never)
    pre = r"Error propagating flow: "
    flow = ofl.Flow(torch.zeros(2, 2, 5, 7))
    good = torch.zeros(2, 3, 5, 7)
    call = flow.propagate
    for bad in ("feat", 3, [good], np.zeros((2, 3, 5, 7), np.float64), good.double(), good.half(), good.bfloat16(), good.to(torch.uint8)):
        with pytest.raises(TypeError, match=pre):
            call(bad, good)
        with pytest.raises(TypeError, match=pre):
            call(good, bad)
    with pytest.raises(TypeError, match=pre):
        call(None)
    for bad in (torch.zeros(5, 7), torch.zeros(1, 2, 3, 5, 7)):
        with pytest.raises(ValueError, match=pre + "Query needs to have 3 or 4 dimensions"):
            call(bad, good)
        with pytest.raises(ValueError, match=pre + "Key needs to have 3 or 4 dimensions"):
            call(good, bad)
    with pytest.raises(ValueError, match=pre + "Query needs to have at least 1 channel"):
        call(torch.zeros(2, 0, 5, 7))
    with pytest.raises(ValueError, match=pre + "Query and key need to have the same number of channels"):
        call(good, torch.zeros(2, 4, 5, 7))
    for bad in (torch.zeros(2, 3, 7, 5), torch.zeros(3, 5, 6)):
        with pytest.raises(ValueError, match=pre + "Key needs to have the H-W shape of the flow"):
            call(good, bad)
    for bad in (torch.zeros(1, 3, 5, 7), torch.zeros(3, 3, 5, 7)):
        with pytest.raises(ValueError, match=pre + "Query needs to have the batch size of the flow"):
            call(bad, good)
    for bad in (1.0, "1", True):
        with pytest.raises(TypeError, match=pre + "Radius needs to be an integer or None"):
            call(good, radius=bad)
    for bad in (0, 5, -1):
        with pytest.raises(ValueError, match=pre + "Radius needs to be None, 1, 2, 3 or 4"):
            call(good, radius=bad)
    for bad in (1, 0, "True"):
        with pytest.raises(TypeError, match=pre + "Consider_mask needs to be boolean"):
            call(good, consider_mask=bad)
    with pytest.raises(ValueError, match=pre):
        ofl.propagate_flow(torch.zeros(2, 2, 5, 7), good[:1])
    with pytest.raises(TypeError, match=pre):
        ofl.propagate_flow(torch.zeros(2, 2, 5, 7), good.double())
    # the bindings check for themselves
    vecs = torch.zeros(2, 2, 5, 7)
    with pytest.raises(ValueError, match="at least one output"):
        _propagate.flow_propagate_grad(vecs, None, good, good, None, torch.zeros(28 * 70, dtype=torch.uint8), vecs, False, False, False)
    with pytest.raises(TypeError, match="float32"):
        _propagate.check_operands(vecs, None, good.double(), good, None)
    with pytest.raises(ValueError, match="flow's shape"):
        _propagate.check_operands(vecs, None, good, good[:1], None)
    with pytest.raises(ValueError, match="same number of channels"):
        _propagate.check_operands(vecs, None, good, good[:, :2], None)
    with pytest.raises(ValueError, match="1, 2, 3 or 4"):
        _propagate.check_operands(vecs, None, good, good, 5)
    assert _propagate.STATS_BYTES == 28 and _propagate.MAX_RADIUS == 4


def test_the_method_and_the_wrapper_are_exported():
    import oflibpytorch_amd as ofl
    assert callable(ofl.Flow.propagate) and callable(ofl.propagate_flow)
    doc = " ".join(ofl.Flow.propagate.__doc__.split())
    assert "never formed" in doc and "not with respect to the mask" in doc and "EMPTY" in doc
    assert "Flow.propagate" in ofl.__doc__ and "propagate_flow" in ofl.__doc__


# ---- the C ABI: declared, exported, and every rejected argument is rejected before any launch -----------------------------------------
def test_c_abi_declarations_and_argument_checks_need_no_gpu():
    from oflibpytorch_amd import _native, _propagate
    names = {"ofl_flow_propagate_global_f32", "ofl_flow_propagate_global_grad_f32", "ofl_flow_propagate_local_f32",
             "ofl_flow_propagate_local_grad_f32"}
    assert names <= set(_native.exported_symbols())
    header = open(_native._build.HEADERS[0]).read()
    for name in names:
        assert (" %s(" % name) in header
    assert any(src.endswith("ofl_propagate.hip") for src in _native._build.SOURCES)
    lib = _propagate._library()
    for name in names:
        assert hasattr(lib, name)                                        # present in the built library
    assert lib.ofl_version() == _native.ABI_VERSION == 36                # names were added, no signature changed
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(4096)               # never dereferenced: every call below is rejected first
    odd, odd8 = ctypes.c_void_p(4098), ctypes.c_void_p(4100)

    def ops(kw):
        d = dict(query=one, query_bs=0, key=one, key_bs=0, c=4, flow=one, flow_bs=0, mask=one, mask_bs=0, n=1, h=4, w=4)
        d.update(kw)
        return d

    def fwd(radius=None, out=one, valid=one, ws=one, **kw):
        d = ops(kw)
        head = (d['query'], d['query_bs'], d['key'], d['key_bs'], d['c'], d['flow'], d['flow_bs'], d['mask'], d['mask_bs'])
        tail = (out, valid, ws, d['n'], d['h'], d['w'], null)
        if radius is None:
            return lib.ofl_flow_propagate_global_f32(*(head + tail))
        return lib.ofl_flow_propagate_local_f32(*(head + (radius,) + tail))

    def bwd(radius=None, ws=one, g=one, scratch=one, dq=one, dk=one, df=one, **kw):
        d = ops(kw)
        head = (d['query'], d['query_bs'], d['key'], d['key_bs'], d['c'], d['flow'], d['flow_bs'], d['mask'], d['mask_bs'])
        tail = (dq, dk, df, d['n'], d['h'], d['w'], null)
        if radius is None:
            return lib.ofl_flow_propagate_global_grad_f32(*(head + (ws, g) + tail))
        return lib.ofl_flow_propagate_local_grad_f32(*(head + (radius, ws, g, scratch) + tail))
    frame = (dict(n=0), dict(n=65536), dict(n=-3), dict(h=0), dict(w=0), dict(h=-1), dict(c=0), dict(c=-2),
             dict(h=65536, w=32768), dict(h=(1 << 24) + 1, w=1), dict(h=1, w=(1 << 24) + 1),
             dict(query=null), dict(key=null), dict(flow=null), dict(query_bs=-1), dict(key_bs=-1), dict(flow_bs=-1), dict(mask_bs=-1),
             dict(query=odd), dict(key=odd), dict(flow=odd))
    for radius in (None, 2):
        for kw in frame + (dict(out=null), dict(out=odd), dict(ws=odd8)):
            assert fwd(radius, **kw) == -3, (radius, kw)
        for kw in frame + (dict(ws=null), dict(g=null), dict(dq=null, dk=null, df=null), dict(ws=odd8), dict(g=odd), dict(dq=odd),
                           dict(dk=odd), dict(df=odd)):
            assert bwd(radius, **kw) == -3, (radius, kw)
    for radius in (0, 5, -1):
        assert fwd(radius) == -3 and bwd(radius) == -3
    assert bwd(2, scratch=null) == -3 and bwd(2, scratch=odd) == -3
