"""CPU tier of Flow.from_matching: the oracle (tests/matching_oracle.py) against the textbook expression in torch float64
and its autograd, five mutants that the comparison must tell apart, the exact-softmax inputs of the GPU tier, the host logic of the API
with the native calls served by the oracle, every argument check that needs no device, and the C ABI's declarations and argument checks.
No device."""
import ctypes

import numpy as np
import pytest
import torch

import matching_oracle as mo

SHAPES = ((5, 7), (9, 11))
N = 2


@pytest.fixture
def gm_native(oracle_native, monkeypatch):
    from oflibpytorch_amd import _matching
    monkeypatch.setattr(_matching, "flow_global_match", mo.fake_flow_global_match)
    monkeypatch.setattr(_matching, "flow_global_match_grad", mo.fake_flow_global_match_grad)
    return _matching


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x).copy())


# ---- the oracle computes the textbook expression ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("c", [1, 5, 16])
@pytest.mark.parametrize("h,w", SHAPES)
def test_float64_evaluation_is_the_textbook_expression_and_its_autograd(h, w, c, ref):
    """A batch of 2: the oracle's float64 evaluation (float64 logits, the streaming chain with its rescales as defined) and its gradients
    against softmax(einsum / sqrt(C)) @ grid - grid in torch float64 and torch's autograd of it, within 1e-12 of each result's scale:
    the running-maximum rescale multiplies S, X and Y by the same factor, so it does not enter the quotient beyond a rounding each."""
    sign = -1.0 if ref == 's' else 1.0
    feat, other = mo.features_general(N, c, h, w)
    g = mo.upstream(N, h, w)
    want = mo.textbook(feat, other, sign, g)
    got = mo.compute(feat, other, sign, wide=True)
    gr = mo.grads(feat, other, sign, g, wide=True)
    for name, a, b in (("out", got['out'], want['out']), ("prob", got['prob'].astype(np.float64), want['prob']),
                       ("d feat", gr['d_feat'], want['d_feat']), ("d other", gr['d_other'], want['d_other'])):
        scale = np.abs(b).max()
        err = np.abs(a - b).max()
        print("%d x %d C %d %s %s: largest |oracle float64 - textbook float64| = %.3e of a scale %.3e" % (h, w, c, ref, name, err, scale))
        assert a.dtype == np.float64 and a.shape == b.shape and scale > 0
        assert err <= (1e-12 if name != "prob" else 2.0 ** -24) * scale, name             # (prob is rounded to float32)
    # the definition's float32 results are the float32-logit chain rounded once, and close to the textbook's
    d = mo.compute(feat, other, sign)
    assert np.array_equal(d['out32'], d['out'].astype(np.float32))
    assert np.abs(d['out'] - want['out']).max() <= 1e-4 * np.abs(want['out']).max()


@pytest.mark.parametrize("mutant", mo.MUTANTS)
def test_mutants_fail_the_comparison(mutant):
    """x and y swapped, the softmax taken over p instead of q, the 1 / sqrt(C) dropped and the sign of 't' not flipped each compute
    another function, whose distance from the textbook's is of the order of the result itself: each must miss by more than a tenth of
    the result's scale, on inputs where the oracle itself is within 1e-12"""
    h, w, c = 5, 7, 5
    feat, other = mo.features_general(N, c, h, w)
    want = mo.textbook(feat, other, 1.0)['out']                                              # a 't' flow
    scale = np.abs(want).max()
    miss = np.abs(mo.compute(feat, other, 1.0, wide=True, mutant=mutant)['out'] - want).max()
    print("%s: misses by %.3f of the scale" % (mutant, miss / scale))
    assert miss > 0.1 * scale
    assert np.abs(mo.compute(feat, other, 1.0, wide=True)['out'] - want).max() <= 1e-12 * scale


def test_a_column_major_walk_is_told_apart_by_bits_only():
    """q walked column-major: on the all-equal family every weight is exactly 1 / Q whatever the order, so the forward has the same bits;
    d feat is a float32 sum of Q different terms, and only its bits tell the order of the walk"""
    n, c, h, w = 1, 16, 5, 13
    feat, other = mo.features_exact('all-equal', n, c, h, w)
    g = mo.upstream(n, h, w)
    walk = mo.column_major(h, w)
    assert sorted(walk) == list(range(h * w)) and walk != list(range(h * w))
    a, b = mo.compute(feat, other, -1.0), mo.compute(feat, other, -1.0, walk=walk)
    assert np.array_equal(a['out32'], b['out32']) and np.array_equal(a['prob'], b['prob'])
    ga, gb = mo.grads(feat, other, -1.0, g), mo.grads(feat, other, -1.0, g, walk=walk)
    differ = int((ga['d_feat'].view(np.uint32) != gb['d_feat'].view(np.uint32)).sum())
    print("column-major walk: %d of %d elements of d feat differ in bits" % (differ, ga['d_feat'].size))
    assert differ > ga['d_feat'].size // 4
    # (the terms of a pixel cancel: sum_q (q - o) = 0 and `other` is the same at every q -- what is left IS the rounding of the walk)
    assert np.abs(ga['d_feat'].astype(np.float64) - gb['d_feat']).max() <= 1e-5 * ga['mag_feat'].max()


@pytest.mark.parametrize("c", [4, 16])
def test_the_exact_inputs_are_what_they_say(c):
    """The bit-for-bit tier of the GPU tests rests on these: every logit is 0 or at most -800, every weight 0, 1/2, 1/Q or 1"""
    g = mo.geometry()
    n, h, w = 3, 5, 13                                                                       # Q = 65: two chunks and a tile, plus one
    q = h * w
    px, py = np.arange(q) % w, np.arange(q) // w
    for kind in ('one-hot', 'two-hot', 'all-equal') + (('rising',) if c == 16 else ()):
        feat, other = mo.features_exact(kind, n, c, h, w)
        assert set(np.unique(feat).tolist()) <= {0.0, 32.0} and set(np.unique(other).tolist()) <= {0.0, -32.0}
        r = mo.compute(feat, other, -1.0)
        s = r['s']
        assert ((s == 0) | (s <= -800)).all(), kind
        wt = r['w']
        if kind == 'one-hot':
            tg = mo.targets(kind, q, c)
            assert set(np.unique(wt).tolist()) == {0.0, 1.0} and np.array_equal(wt.sum(2), np.ones((n, q)))
            assert q - 1 in tg and (c == 4 or {0, g["kChunkQ"] - 1, g["kChunkQ"], g["kTileP"] - 1, g["kTileP"]} <= set(tg))
            hit = wt.argmax(2)
            assert set(np.unique(hit).tolist()) == set(tg)                                   # every named position is somebody's match
            assert np.array_equal(r['out32'][:, 0].reshape(n, q), (px[hit] - px[None]).astype(np.float32))
            assert np.array_equal(r['out32'][:, 1].reshape(n, q), (py[hit] - py[None]).astype(np.float32))
            assert np.array_equal(r['prob'], np.ones((n, h, w), np.float32))
        elif kind == 'two-hot':
            assert set(np.unique(wt).tolist()) == {0.0, 0.5} and ((wt == 0.5).sum(2) == 2).all()
            first, second = wt.argmax(2), q - 1 - wt[:, :, ::-1].argmax(2)
            assert (first // g["kChunkQ"] != second // g["kChunkQ"]).all()                   # in different chunks
            assert np.array_equal(r['prob'], np.full((n, h, w), 0.5, np.float32))
        elif kind == 'all-equal':
            assert np.array_equal(wt, np.full_like(wt, 1.0 / q)) and np.array_equal(r['S'], np.full((n, q), float(q)))
            f2, o2 = mo.features_exact(kind, 1, c, 8, 8)                                     # Q a power of two: 1 / Q is exact
            assert np.array_equal(mo.compute(f2, o2, -1.0)['w'] * 64.0, np.ones((1, 64, 64)))
        else:
            assert set(np.unique(wt).tolist()) == {0.0, 1.0}
            rises = np.zeros((n, q), int)
            m = s[:, :, 0].copy()
            for pos in range(1, q):
                up = s[:, :, pos] > m
                assert (s[:, :, pos][up] - m[up] >= 800).all()
                rises += up
                m = np.maximum(m, s[:, :, pos])
            assert set(np.unique(rises).tolist()) == {1, 2}                                  # word A rises twice, word B once and then falls
            assert np.array_equal(r['m'], np.zeros((n, q), np.float32))


def test_non_finite_values_follow_ieee():
    n, c, h, w = 1, 3, 3, 4
    feat, other = (a.copy() for a in mo.features_general(n, c, h, w))
    clean = mo.compute(feat, other, -1.0)
    f = feat.copy()
    f[0, 1, 1, 2] = np.nan                                                                   # pixel 6
    r = mo.compute(f, other, -1.0)
    bad = np.zeros((n, 2, h, w), bool)
    bad[:, :, 1, 2] = True
    assert np.isnan(r['out32'][bad]).all() and np.array_equal(r['out32'][~bad], clean['out32'][~bad]) and np.isnan(r['prob'][0, 1, 2])
    o = other.copy()
    o[0, 0, 2, 1] = np.nan
    assert np.isnan(mo.compute(feat, o, -1.0)['out32']).all()
    o = other.copy()
    o[0, 0, 2, 1] = np.inf                                                                   # logits of +inf where feat_0(p) > 0: inf - inf
    r = mo.compute(feat, o, -1.0)
    pos = (feat[0, 0] > 0)
    neg = (feat[0, 0] < 0)
    assert pos.any() and neg.any()
    assert np.isnan(r['out32'][0, 0][pos]).all() and np.isfinite(r['out32'][0, 0][neg]).all()
    assert (r['w'][0].reshape(h, w, h * w)[neg][:, 2 * w + 1] == 0).all()                    # a logit of -inf: a weight of exactly 0


# ---- the host logic of the API, the oracle in the bindings' place ---------------------------------------------------------------------
@pytest.mark.parametrize("ref", ['s', 't', None])
def test_shapes_values_ref_mask_and_prob(gm_native, ref):
    import oflibpytorch_amd as ofl
    (h, w), c = SHAPES[0], 5
    feat, other = mo.features_general(N, c, h, w)
    sign = -1.0 if ref == 's' else 1.0
    want = mo.compute(feat, other, sign)
    mask = np.random.RandomState(5).uniform(size=(N, h, w)) > 0.3
    flow = ofl.Flow.from_matching(_t(feat), _t(other), ref, _t(mask))
    assert isinstance(flow, ofl.Flow) and flow.ref == ('t' if ref is None else ref) and flow.shape == (N, h, w)
    assert flow.vecs.dtype == torch.float32 and not flow.vecs.requires_grad and flow.device == torch.device('cpu')
    assert np.array_equal(flow.vecs.numpy(), want['out32']) and np.array_equal(flow.mask.numpy(), mask)
    assert bool(ofl.Flow.from_matching(_t(feat), _t(other), ref).mask.all())
    for flag in (None, False):
        assert isinstance(ofl.Flow.from_matching(_t(feat), _t(other), ref, return_prob=flag), ofl.Flow)
    res = ofl.Flow.from_matching(_t(feat), _t(other), ref, return_prob=True)
    assert isinstance(res, tuple) and len(res) == 2 and isinstance(res[0], ofl.Flow)
    assert res[1].dtype == torch.float32 and res[1].shape == (N, h, w) and np.array_equal(res[1].numpy(), want['prob'])
    assert np.array_equal(res[0].vecs.numpy(), want['out32'])
    # a 3-dimensional input is a batch of one; the tensor wrapper gives back the input's dimension count
    one = ofl.Flow.from_matching(_t(feat[1]), _t(other[1]), ref)
    assert one.shape == (1, h, w) and np.array_equal(one.vecs.numpy()[0], want['out32'][1])
    ref2 = 't' if ref is None else ref
    got = ofl.global_matching_flow(_t(feat[1]), _t(other[1]), ref2)
    assert got.shape == (2, h, w) and np.array_equal(got.numpy(), want['out32'][1])
    got, prob = ofl.global_matching_flow(_t(feat), _t(other), ref2, return_prob=True)
    assert got.shape == (N, 2, h, w) and np.array_equal(got.numpy(), want['out32']) and np.array_equal(prob.numpy(), want['prob'])
    got, prob = ofl.global_matching_flow(_t(feat[0]), _t(other[0]), ref2, return_prob=True)
    assert got.shape == (2, h, w) and prob.shape == (h, w)


@pytest.mark.parametrize("need", ["none", "feat", "other", "both"])
def test_requires_grad_routing(gm_native, monkeypatch, need):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _autograd
    h, w, c = 5, 7, 5
    feat, other = mo.features_general(N, c, h, w)
    g = mo.upstream(N, h, w)
    calls = []
    real = mo.fake_flow_global_match_grad

    def spy(feat, other, flow_sign, stats, grad_out, want_feat=True, want_other=True):
        calls.append((want_feat, want_other))
        return real(feat, other, flow_sign, stats, grad_out, want_feat, want_other)
    monkeypatch.setattr(gm_native, "flow_global_match_grad", spy)
    ft = _t(feat).requires_grad_(need in ("feat", "both"))
    ot = _t(other).requires_grad_(need in ("other", "both"))
    flow, prob = ofl.Flow.from_matching(ft, ot, 's', return_prob=True)
    assert issubclass(_autograd.GlobalMatchFn, torch.autograd.Function)
    assert not prob.requires_grad
    if need == "none":
        assert not flow.vecs.requires_grad and flow.vecs.grad_fn is None
        return
    assert flow.vecs.requires_grad and type(flow.vecs.grad_fn).__name__ == "GlobalMatchFnBackward"
    flow.vecs.backward(_t(g))
    assert calls == [(need in ("feat", "both"), need in ("other", "both"))]
    want = mo.grads(feat, other, -1.0, g)
    for t, name, wanted in ((ft, 'd_feat', need in ("feat", "both")), (ot, 'd_other', need in ("other", "both"))):
        if wanted:
            assert t.grad.dtype == torch.float32 and np.array_equal(t.grad.numpy(), want[name])
        else:
            assert t.grad is None
    with torch.no_grad():
        assert not ofl.Flow.from_matching(ft, ot, 's').vecs.requires_grad
    # a C-H-W operand gets a C-H-W gradient
    f3 = _t(feat[0]).requires_grad_(True)
    ofl.Flow.from_matching(f3, _t(other[0]), 's').vecs.backward(_t(g[:1]))
    assert f3.grad.shape == f3.shape and np.array_equal(f3.grad.numpy(), mo.grads(feat[:1], other[:1], -1.0, g[:1])['d_feat'][0])


def test_api_checks_and_their_messages(oracle_native, monkeypatch):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _matching

    def never(*args, **kw):
        raise AssertionError("the checks come before the kernel")
    monkeypatch.setattr(_matching, "flow_global_match", never)
    monkeypatch.setattr(_matching, "global_match", never)
    pre = r"Error matching flow: "
    good = torch.zeros(2, 3, 5, 7)
    call = ofl.Flow.from_matching
    for bad in ("feat", 3, None, [good], np.zeros((2, 3, 5, 7), np.float32), good.double(), good.half(), good.bfloat16(), good.to(torch.uint8)):
        with pytest.raises(TypeError, match=pre):
            call(bad, good)
        with pytest.raises(TypeError, match=pre):
            call(good, bad)
    for bad in (1, 0, "True"):
        with pytest.raises(TypeError, match=pre + "Return_prob needs to be boolean"):
            call(good, good, return_prob=bad)
    for bad in (torch.zeros(5, 7), torch.zeros(1, 2, 3, 5, 7)):
        with pytest.raises(ValueError, match=pre + "Feat needs to have 3 or 4 dimensions"):
            call(bad, bad)
    for bad in (torch.zeros(2, 3, 7, 5), torch.zeros(2, 4, 5, 7), torch.zeros(1, 3, 5, 7), torch.zeros(3, 5, 7)):
        with pytest.raises(ValueError, match=pre + "Feat and other need to have the same shape"):
            call(good, bad)
    for bad in (torch.zeros(2, 0, 5, 7), torch.zeros(2, 3, 0, 7), torch.zeros(2, 3, 5, 0), torch.zeros(0, 3, 5, 7), torch.zeros(3, 0, 7)):
        with pytest.raises(ValueError, match=pre + "Feat and other must not be empty"):
            call(bad, bad)
    for bad in ('x', 'st', 3, ['s']):
        with pytest.raises(ValueError, match=pre + "Ref needs to be 's' or 't'"):
            call(good, good, bad)
    with pytest.raises(ValueError, match=pre):
        ofl.global_matching_flow(good, good[:1], 's')
    with pytest.raises(TypeError, match=pre):
        ofl.global_matching_flow(good, good.double(), 's')
    # the bindings check for themselves
    with pytest.raises(ValueError, match="at least one output"):
        _matching.flow_global_match_grad(good, good, -1.0, torch.zeros(28 * 70, dtype=torch.uint8), torch.zeros(2, 2, 5, 7), False, False)
    with pytest.raises(TypeError, match="float32"):
        _matching.check_features(good.double(), good)
    with pytest.raises(ValueError, match="same shape"):
        _matching.check_features(good, good[:1])
    assert _matching.STATS_BYTES == 28


def test_the_method_and_the_wrapper_are_exported():
    import oflibpytorch_amd as ofl
    assert callable(ofl.Flow.from_matching) and callable(ofl.global_matching_flow)
    doc = " ".join(ofl.Flow.from_matching.__doc__.split())
    assert "never formed" in doc and "NOT through the probability" in doc
    assert "from_matching" in ofl.__doc__ and "global_matching_flow" in ofl.__doc__


# ---- the C ABI: declared, exported, and every rejected argument is rejected before any launch -----------------------------------------
def test_c_abi_declarations_and_argument_checks_need_no_gpu():
    from oflibpytorch_amd import _matching, _native
    names = {"ofl_flow_global_match_f32", "ofl_flow_global_match_grad_f32"}
    assert names <= set(_native.exported_symbols())
    header = open(_native._build.HEADERS[0]).read()
    for name in names:
        assert (" %s(" % name) in header
    assert any(src.endswith("ofl_matching.hip") for src in _native._build.SOURCES)
    lib = _matching._library()
    for name in names:
        assert hasattr(lib, name)                                        # present in the built library
    assert lib.ofl_version() == _native.ABI_VERSION == 36                # names were added, no signature changed
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(4096)               # never dereferenced: every call below is rejected first
    odd, odd8 = ctypes.c_void_p(4098), ctypes.c_void_p(4100)

    def fwd(feat=one, feat_bs=0, other=one, other_bs=0, c=4, sign=-1.0, out=one, prob=one, ws=one, n=1, h=4, w=4):
        return lib.ofl_flow_global_match_f32(feat, feat_bs, other, other_bs, c, sign, out, prob, ws, n, h, w, null)

    def bwd(feat=one, feat_bs=0, other=one, other_bs=0, c=4, sign=-1.0, ws=one, g=one, df=one, do=one, n=1, h=4, w=4):
        return lib.ofl_flow_global_match_grad_f32(feat, feat_bs, other, other_bs, c, sign, ws, g, df, do, n, h, w, null)
    frame = (dict(n=0), dict(n=65536), dict(n=-3), dict(h=0), dict(w=0), dict(h=-1), dict(c=0), dict(c=-2), dict(sign=0.0), dict(sign=2.0),
             dict(h=65536, w=32768), dict(h=(1 << 24) + 1, w=1), dict(h=1, w=(1 << 24) + 1),
             dict(feat=null), dict(other=null), dict(feat_bs=-1), dict(other_bs=-1), dict(feat=odd), dict(other=odd))
    for kw in frame + (dict(out=null), dict(out=odd), dict(prob=odd), dict(ws=odd8)):
        assert fwd(**kw) == -3, kw
    for kw in frame + (dict(ws=null), dict(g=null), dict(df=null, do=null), dict(ws=odd8), dict(g=odd), dict(df=odd), dict(do=odd)):
        assert bwd(**kw) == -3, kw
