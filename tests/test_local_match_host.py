"""CPU tier of Flow.match_local: the oracle (tests/local_match_oracle.py) against GMFlow's expression written
independently in torch float64 -- an unfold-style window of the warped tensor, the positions outside the frame at -inf, the expected
offset added to the flow -- and torch's autograd of it, six mutants that the comparison must tell apart, the exact-softmax inputs of the
GPU tier, the host logic of the API with the native calls served by the oracle, every argument check that needs no device, and the C
ABI's declarations and argument checks.  No device."""
import ctypes

import numpy as np
import pytest
import torch

import local_match_oracle as lo

SHAPES = ((5, 7), (9, 11))
N = 2


@pytest.fixture
def lm_native(oracle_native, monkeypatch):
    from oflibpytorch_amd import _local_match
    monkeypatch.setattr(_local_match, "flow_local_match", lo.fake_flow_local_match)
    monkeypatch.setattr(_local_match, "flow_local_match_grad", lo.fake_flow_local_match_grad)
    return _local_match


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x).copy())


def _mask(n, h, w):
    m = np.random.RandomState(23 + h + w).uniform(size=(n, h, w)) > 0.3
    assert m.any((1, 2)).all() and not m.all()
    return m


def _compare(h, w, radius, c, ref, masked, mutant=None):
    """{name: (largest |oracle float64 - textbook float64|, the textbook's scale)} of the forward and the three gradients plus d other"""
    feat, other = lo.features_general(N, c, h, w)
    a, g = lo.vectors_general(N, h, w), lo.upstream(N, h, w)
    mask = _mask(N, h, w) if masked else None
    usable = lo.usable_of(a, mask, ref)
    assert usable.any() and not usable.all()
    want = lo.textbook(a, usable, feat, other, ref, radius, g)
    assert np.isfinite(want['out']).all()
    got = lo.compute(a, mask, feat, other, ref, radius, wide=True, mutant=mutant)
    gr = lo.grads(a, mask, feat, other, ref, radius, g, wide=True, mutant=mutant, res=got)
    out = {}
    for name, x, y in (("out", got['out'], want['out']), ("prob", (1.0 / got['S']), want['prob']), ("d feat", gr['d_feat'], want['d_feat']),
                       ("d W", gr['d_w'], want['d_warped']), ("d other", gr['d_other'], want['d_other']),
                       ("d flow", gr['d_flow'], want['d_flow'])):
        assert x.dtype == np.float64 and x.shape == y.shape, name
        out[name] = (np.abs(x - y).max(), np.abs(y).max())
    return out


# ---- the oracle computes the textbook expression --------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("ref", lo.REFS)
@pytest.mark.parametrize("c", [1, 5, 16])
@pytest.mark.parametrize("radius", lo.RADII)
@pytest.mark.parametrize("h,w", SHAPES)
def test_float64_evaluation_is_the_textbook_expression_and_its_autograd(h, w, radius, c, ref, masked):
    """A batch of 2: the oracle's float64 evaluation and its gradients against the torch float64 expression and torch's autograd of it,
    within 1e-12 of each result's scale (measured over all cases: at most 3e-15 of the scale)"""
    for name, (err, scale) in _compare(h, w, radius, c, ref, masked).items():
        print("%d x %d r %d C %d %s %s: largest |oracle float64 - textbook float64| = %.3e of a scale %.3e" % (h, w, radius, c, ref, name,
                                                                                                                  err, scale))
        assert scale > 0 and err <= 1e-12 * scale, name
    # the definition's float32 result is its float64 sum rounded once, and close to the textbook's
    feat, other = lo.features_general(N, c, h, w)
    a = lo.vectors_general(N, h, w)
    d = lo.compute(a, _mask(N, h, w) if masked else None, feat, other, ref, radius)
    assert np.array_equal(d['out32'], d['out'].astype(np.float32)) and d['m'].dtype == np.float32


WHERE = {"pad_zero": "out", "unusable_excluded": "out", "over_c": "out", "swap_xy": "out", "t_sign": "out", "no_identity": "d flow"}


@pytest.mark.parametrize("mutant", lo.MUTANTS)
def test_mutants_fail_the_comparison(mutant):
    """Each mutant misses the textbook by more than 0.1 of the scale of the result named in WHERE -- out-of-frame positions given the
    logit 0, unusable positions excluded, 1 / C for 1 / sqrt(C), dx and dy swapped, the sign of 't' not flipped, the identity term of
    d flow dropped -- measured on the expected offset itself (the result minus the flow) for the forward"""
    h, w, c, radius, ref = 9, 11, 16, 2, 't'
    feat, other = lo.features_general(N, c, h, w)
    a, g = lo.vectors_general(N, h, w), lo.upstream(N, h, w)
    mask = _mask(N, h, w)
    usable = lo.usable_of(a, mask, ref)
    want = lo.textbook(a, usable, feat, other, ref, radius, g)
    got = lo.compute(a, mask, feat, other, ref, radius, wide=True, mutant=mutant)
    gr = lo.grads(a, mask, feat, other, ref, radius, g, wide=True, mutant=mutant, res=got)
    if WHERE[mutant] == "out":
        move = want['out'] - a.astype(np.float64)                                            # E[o] up to its sign
        err, scale = np.abs(got['out'] - want['out']).max(), np.abs(move).max()
    else:
        err, scale = np.abs(gr['d_flow'] - want['d_flow']).max(), np.abs(want['d_flow']).max()
    print("%s: misses by %.3f of the scale" % (mutant, err / scale))
    assert err > 0.1 * scale
    clean = _compare(h, w, radius, c, ref, True)
    assert all(e <= 1e-12 * s for e, s in clean.values())


@pytest.mark.parametrize("ref", lo.REFS)
@pytest.mark.parametrize("radius", [1, 4])
@pytest.mark.parametrize("c", [4, 16])
def test_the_exact_inputs_are_what_they_say(c, radius, ref):
    """The exact families on 11 x 13: entries in {0, +-32}, every logit difference 0 or at most -1024, so that every weight is a ratio of
    small integers under any correct exp; and the conditions the GPU tier asserts of them"""
    n, h, w = 3, 11, 13
    a = lo.vectors_integer(n, h, w, ref)
    mask = lo.masks(n, h, w)['single']
    for kind in lo.exact_kinds(c):
        feat, other = lo.features_exact(kind, a, mask, ref, c, radius)
        assert set(np.unique(feat)) <= {0.0, 32.0} and set(np.unique(other)) <= ({0.0, 32.0} if kind == 'two-hot' else {0.0, -32.0})
        r = lo.compute(a, mask, feat, other, ref, radius)
        s = r['s']
        assert kind == 'two-hot' or ((s == 0) | (s <= -1024)).all()
        d = np.where(r['part'], s - r['m'][:, None], 0)
        assert ((d == 0) | (d <= -1024)).all() and (s == np.round(s)).all()                 # every difference from the maximum
        e = np.exp(s.astype(np.float64) - r['m'].astype(np.float64)[:, None])
        assert ((e == 1) | (e == 0)).all()
        assert not r['usable'].all() and not r['part'].all()
        if kind == 'one-hot':
            assert np.abs(r['out32'] - a).max() >= 1.0                                     # some vector moves by at least 1 px
        if kind == 'all-equal':
            assert np.array_equal(r['S'], r['terms'].astype(np.float64))                    # every weight is 1 / T
        if kind == 'two-hot':
            two = np.broadcast_to((r['S'] == 2)[:, None], r['w'].shape)
            assert (r['w'] == 0.5).any() and np.isin(r['w'][two], (0.0, 0.5)).all()          # two matches: weights of exactly 1/2
            assert ((r['w'] == 0.5).sum(1)[r['S'] == 2] == 2).all()
        if kind == 'rising':
            rises = np.zeros(r['m'].shape, int)
            cur = np.full(r['m'].shape, np.nan, np.float32)
            for o in range(s.shape[1]):
                up = r['part'][:, o] & (np.isnan(cur) | (s[:, o] > cur))
                rises += up & ~np.isnan(cur)
                cur = np.where(up, s[:, o], cur)
            assert rises.max() >= 2
    # an unusable position inside the frame whose logit +0 ties with the maximum
    feat, other = lo.features_exact('one-hot', a, mask, ref, c, radius)
    r = lo.compute(a, mask, feat, other, ref, radius)
    un = np.stack([lo.cvo._shifted(~r['usable'], radius, dy, dx) for dy, dx in lo.offsets(radius)], 1)
    assert (un & r['part'] & (r['s'] == 0) & (r['m'][:, None] == 0)).any()
    far = lo.usable_of(a, None, ref)
    assert not far.all()                                                                     # a vector pointing wholly out of the frame


# ---- the host logic of the API, the native calls served by the oracle ----------------------------------------------------------------
def test_shapes_values_ref_mask_and_prob(lm_native):
    import oflibpytorch_amd as ofl
    (h, w), c, radius = SHAPES[0], 5, 2
    feat, other = lo.features_general(N, c, h, w)
    vec, mask = lo.vectors_general(N, h, w), _mask(N, h, w)
    for ref in lo.REFS:
        want = lo.compute(vec, mask, feat, other, ref, radius)
        flow = ofl.Flow(_t(vec), ref, _t(mask))
        res = flow.match_local(_t(feat), _t(other), radius)
        assert isinstance(res, ofl.Flow) and res.ref == ref and res.shape == (N, h, w) and res.device == flow.device
        assert res.vecs.dtype == torch.float32 and not res.vecs.requires_grad
        assert np.array_equal(res.vecs.numpy(), want['out32']) and np.array_equal(res.mask.numpy(), mask)
        res, prob = flow.match_local(feat.copy(), other.copy(), radius, return_prob=True)
        assert np.array_equal(res.vecs.numpy(), want['out32']) and prob.shape == (N, h, w) and np.array_equal(prob.numpy(), want['prob'])
        free = lo.compute(vec, None, feat, other, ref, radius)
        res = flow.match_local(_t(feat), _t(other), radius, consider_mask=False)
        assert np.array_equal(res.vecs.numpy(), free['out32']) and np.array_equal(res.mask.numpy(), mask)
        one = lo.compute(vec, mask, feat[0], other[0], ref, radius)
        assert np.array_equal(flow.match_local(_t(feat[0]), _t(other[0]), radius).vecs.numpy(), one['out32'])
        got = ofl.local_matching_flow(_t(vec), _t(feat), _t(other), ref, radius, mask=_t(mask))
        assert isinstance(got, torch.Tensor) and np.array_equal(got.numpy(), want['out32'])
        got, prob = ofl.local_matching_flow(_t(vec[0]), _t(feat[0]), _t(other[0]), ref, radius, return_prob=True)
        assert got.shape == (2, h, w) and prob.shape == (h, w)
        assert np.array_equal(got.numpy(), lo.compute(vec[:1], None, feat[:1], other[:1], ref, radius)['out32'][0])
    # the default radius is 4
    assert np.array_equal(ofl.Flow(_t(vec), 's').match_local(_t(feat), _t(other)).vecs.numpy(),
                          lo.compute(vec, None, feat, other, 's', 4)['out32'])


def test_requires_grad_routing_of_the_features(lm_native, monkeypatch):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _autograd
    h, w, c, radius = 5, 7, 5, 1
    feat, other = lo.features_general(N, c, h, w)
    vec, g, mask = lo.vectors_general(N, h, w), lo.upstream(N, h, w), _mask(N, h, w)
    calls = []
    real = lo.fake_flow_local_match_grad

    def spy(*args, want_feat=True, want_warped=True):
        calls.append((want_feat, want_warped))
        return real(*args, want_feat=want_feat, want_warped=want_warped)
    monkeypatch.setattr(lm_native, "flow_local_match_grad", spy)
    assert issubclass(_autograd.LocalMatchFn, torch.autograd.Function)
    res = ofl.Flow(_t(vec), 't', _t(mask)).match_local(_t(feat), _t(other), radius)
    assert not res.vecs.requires_grad and res.vecs.grad_fn is None
    ft = _t(feat).requires_grad_(True)
    res, prob = ofl.Flow(_t(vec), 't', _t(mask)).match_local(ft, _t(other), radius, return_prob=True)
    assert type(res.vecs.grad_fn).__name__ == "LocalMatchFnBackward" and not prob.requires_grad
    res.vecs.backward(_t(g))
    assert calls == [(True, False)]                                                          # no d W: nothing of the warp's backward runs
    assert np.array_equal(ft.grad.numpy(), lo.grads(vec, mask, feat, other, 't', radius, g)['d_feat'])
    f3 = _t(feat[0]).requires_grad_(True)                                                    # C-H-W: a C-H-W gradient, the batch summed
    ofl.Flow(_t(vec), 's', _t(mask)).match_local(f3, _t(other), radius).vecs.backward(_t(g))
    assert f3.grad.shape == f3.shape
    assert np.array_equal(f3.grad.numpy(), lo.grads(vec, mask, feat[:1], other, 's', radius, g)['d_feat'].sum(0))
    with torch.no_grad():
        assert not ofl.Flow(_t(vec), 't').match_local(ft, _t(other), radius).vecs.requires_grad


@pytest.mark.parametrize("need", ["other", "flow", "all"])
@pytest.mark.parametrize("ref", lo.REFS)
def test_the_whole_backward_on_the_host(lm_native, monkeypatch, ref, need):
    """d feat and d W from the oracle, d other and d flow from its float64 backward of the warp in place of `_native.warp_bwd_grad`, the
    chain vectors and the gate from cost_volume_oracle.py: against torch's float64 autograd of the definition; d flow is g plus the
    warp's part, g itself where the pixel is not usable; what needs no gradient costs no call.  The bar is 1e-5 of the scale: the float32
    sums of at most D + C = 30 terms, each within 2^-24 of the sum of their magnitudes, against a float64 reference"""
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _cost_volume, _native
    calls = []

    def fake_warp_bwd_grad(flow, src, grad_out, *, flow_sign=1.0, g_scale=1.0, want_src=True, want_flow=True):
        calls.append((flow_sign, want_src, want_flow))
        assert src.dim() == 4 and g_scale == 1.0
        d_other, d_flow = lo.chain(flow.detach().numpy(), src.detach().numpy(), grad_out.numpy(), lo._ref_of(flow_sign))
        return (torch.from_numpy(d_other).float() if want_src else None), (torch.from_numpy(d_flow).float() if want_flow else None)
    gates = []

    def gate(*args):
        gates.append(1)
        return lo.cvo.fake_flow_cost_volume_gate(*args)
    monkeypatch.setattr(_native, "warp_bwd_grad", fake_warp_bwd_grad)
    monkeypatch.setattr(_cost_volume, "flow_cost_volume_chain", lo.cvo.fake_flow_cost_volume_chain)
    monkeypatch.setattr(_cost_volume, "flow_cost_volume_gate", gate)
    h, w, c, radius = 9, 11, 5, 2
    feat, other = lo.features_general(N, c, h, w)
    vec, g, mask = lo.vectors_general(N, h, w), lo.upstream(N, h, w), _mask(N, h, w)
    usable = lo.usable_of(vec, mask, ref)
    want = lo.textbook(vec, usable, feat, other, ref, radius, g)
    wants = {k: need in (k, "all") for k in ("feat", "other", "flow")}
    ft, ot, vt = _t(feat).requires_grad_(wants["feat"]), _t(other).requires_grad_(wants["other"]), _t(vec).requires_grad_(wants["flow"])
    res = ofl.Flow(vt, ref, _t(mask)).match_local(ft, ot, radius)
    assert type(res.vecs.grad_fn).__name__ == "LocalMatchFnBackward" and np.array_equal(res.mask.numpy(), mask)
    res.vecs.backward(_t(g))
    assert calls == [(lo.sign_of(ref), wants["other"], wants["flow"])] and len(gates) == int(wants["flow"])
    for name, t, key in (("feat", ft, 'd_feat'), ("other", ot, 'd_other'), ("flow", vt, 'd_flow')):
        if not wants[name]:
            assert t.grad is None
            continue
        err, scale = np.abs(t.grad.numpy() - want[key]).max(), np.abs(want[key]).max()
        assert t.grad.dtype == torch.float32 and err <= 1e-5 * scale, (name, err, scale)
    if wants["flow"]:
        un = ~np.broadcast_to(usable[:, None], g.shape)
        assert un.any() and np.array_equal(vt.grad.numpy()[un], g[un])


# ---- checks that need no device: they fail where the names do not exist ----------------------------------------------------------------
def test_the_new_names_are_exported():
    import oflibpytorch_amd as ofl
    assert callable(ofl.Flow.match_local) and callable(ofl.local_matching_flow)
    doc = " ".join(ofl.Flow.match_local.__doc__.split())
    assert "OUTSIDE the frame takes no part" in doc and "never written" in doc
    assert "Flow.match_local" in ofl.__doc__ and "local_matching_flow" in ofl.__doc__


def test_api_checks_and_their_messages(oracle_native, monkeypatch):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _local_match

    def never(*args, **kw):
        raise AssertionError("the checks come before the kernel")
    monkeypatch.setattr(_local_match, "flow_local_match", never)
    monkeypatch.setattr(_local_match, "local_match", never)
    pre = r"Error matching flow locally: "
    flow = ofl.Flow(torch.zeros(2, 2, 5, 7))
    good = torch.zeros(2, 3, 5, 7)
    call = flow.match_local
    for bad in ("feat", 3, [good], None, np.zeros((2, 3, 5, 7), np.float64), good.double(), good.half(), good.bfloat16()):
        with pytest.raises(TypeError, match=pre):
            call(bad, good)
        with pytest.raises(TypeError, match=pre):
            call(good, bad)
    for bad in (torch.zeros(5, 7), torch.zeros(1, 2, 3, 5, 7)):
        with pytest.raises(ValueError, match=pre + "Feat needs to have 3 or 4 dimensions"):
            call(bad, good)
    with pytest.raises(ValueError, match=pre + "Feat needs to have at least 1 channel"):
        call(torch.zeros(2, 0, 5, 7), good)
    with pytest.raises(ValueError, match=pre + "Feat and other need to have the same number of channels"):
        call(good, torch.zeros(2, 4, 5, 7))
    for bad in (torch.zeros(2, 3, 7, 5), torch.zeros(3, 5, 6)):
        with pytest.raises(ValueError, match=pre + "Other needs to have the H-W shape of the flow"):
            call(good, bad)
    for bad in (torch.zeros(1, 3, 5, 7), torch.zeros(3, 3, 5, 7)):
        with pytest.raises(ValueError, match=pre + "Feat needs to have the batch size of the flow"):
            call(bad, good)
    with pytest.raises(ValueError, match=pre + "Flow field needs to be at least 2 pixels high and wide"):
        ofl.Flow(torch.zeros(1, 2, 1, 7)).match_local(torch.zeros(3, 1, 7), torch.zeros(3, 1, 7))
    for bad in (1.0, "1", True):
        with pytest.raises(TypeError, match=pre + "Radius needs to be an integer"):
            call(good, good, radius=bad)
    for bad in (0, 5, -1):
        with pytest.raises(ValueError, match=pre + "Radius needs to be 1, 2, 3 or 4"):
            call(good, good, radius=bad)
    for bad in (1, 0, "True"):
        with pytest.raises(TypeError, match=pre + "Consider_mask needs to be boolean"):
            call(good, good, consider_mask=bad)
        with pytest.raises(TypeError, match=pre + "Return_prob needs to be boolean"):
            call(good, good, return_prob=bad)
    with pytest.raises(ValueError, match=pre):
        ofl.local_matching_flow(torch.zeros(2, 2, 5, 7), good, good[:, :2], 't')
    with pytest.raises(TypeError, match=pre):
        ofl.local_matching_flow(torch.zeros(2, 2, 5, 7), good.double(), good, 't')
    # the bindings check for themselves
    vecs = torch.zeros(2, 2, 5, 7)
    with pytest.raises(ValueError, match="at least one output"):
        _local_match.flow_local_match_grad(vecs, None, good, good, 1.0, 2, torch.zeros(28 * 70, dtype=torch.uint8), vecs, False, False)
    with pytest.raises(TypeError, match="float32"):
        _local_match.check_operands(vecs, good.double(), good, 2)
    with pytest.raises(ValueError, match="flow's shape"):
        _local_match.check_operands(vecs, good, good[:, :, :4], 2)
    with pytest.raises(ValueError, match="same number of channels"):
        _local_match.check_operands(vecs, good, good[:, :2], 2)
    with pytest.raises(ValueError, match="1, 2, 3 or 4"):
        _local_match.check_operands(vecs, good, good, 5)
    assert _local_match.STATS_BYTES == 28 and _local_match.MAX_RADIUS == 4 and _local_match.RADIUS == 4


# ---- the C ABI: declared, exported, and every rejected argument is rejected before any launch -----------------------------------------
def test_c_abi_declarations_and_argument_checks_need_no_gpu():
    from oflibpytorch_amd import _local_match, _native
    names = {"ofl_flow_local_match_f32", "ofl_flow_local_match_grad_f32"}
    assert names <= set(_native.exported_symbols())
    header = open(_native._build.HEADERS[0]).read()
    for name in names:
        assert (" %s(" % name) in header
    assert any(src.endswith("ofl_local_match.hip") for src in _native._build.SOURCES)
    lib = _local_match._library()
    assert lib.ofl_version() == _native.ABI_VERSION == 36                # names were added, no signature changed
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(4096)               # never dereferenced: every call below is rejected first
    odd, odd8 = ctypes.c_void_p(4098), ctypes.c_void_p(4100)

    def head(kw):
        d = dict(flow=one, flow_bs=0, half=0, mask=one, mask_bs=0, feat=one, feat_bs=0, other=one, other_bs=0, c=4, sign=1.0, radius=2,
                 n=1, h=4, w=4)
        d.update(kw)
        return d, (d['flow'], d['flow_bs'], d['half'], d['mask'], d['mask_bs'], d['feat'], d['feat_bs'], d['other'], d['other_bs'], d['c'],
                   d['sign'], d['radius'])

    def fwd(out=one, prob=one, ws=one, **kw):
        d, ops = head(kw)
        return lib.ofl_flow_local_match_f32(*(ops + (out, prob, ws, d['n'], d['h'], d['w'], null)))

    def bwd(ws=one, g=one, scratch=one, df=one, dw=one, **kw):
        d, ops = head(kw)
        return lib.ofl_flow_local_match_grad_f32(*(ops + (ws, g, scratch, df, dw, d['n'], d['h'], d['w'], null)))
    frame = (dict(n=0), dict(n=65536), dict(h=1), dict(w=1), dict(h=0), dict(c=0), dict(h=65536, w=32768), dict(flow=null), dict(feat=null),
             dict(other=null), dict(flow_bs=-1), dict(mask_bs=-1), dict(feat_bs=-1), dict(other_bs=-1), dict(flow=odd), dict(feat=odd),
             dict(other=odd), dict(half=2), dict(sign=0.5), dict(sign=0.0), dict(radius=0), dict(radius=5), dict(radius=-1),
             dict(flow=ctypes.c_void_p(4097), half=1))
    for kw in frame + (dict(out=null), dict(out=odd), dict(prob=odd), dict(ws=odd8)):
        assert fwd(**kw) == -3, kw
    for kw in frame + (dict(ws=null), dict(g=null), dict(scratch=null), dict(df=null, dw=null), dict(ws=odd8), dict(g=odd),
                       dict(scratch=odd), dict(df=odd), dict(dw=odd)):
        assert bwd(**kw) == -3, kw
