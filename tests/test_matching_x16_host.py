"""CPU tier of Flow.from_matching on fp16 / bf16 features: the dispatch by dtype with the bindings served by the oracles,
which pairs of dtypes are accepted and which refused and with what message, the result's type, shape and `prob`, the gradients' dtypes and
shapes, what the graph keeps, that float32 features still take the old binding; the oracle module's own claims (the inputs, the exact
families on the new borders, the bars against the mutants); the C ABI's declarations and argument checks.  No device."""
import ctypes

import numpy as np
import pytest
import torch

import matching_oracle as mo
import matching_x16_oracle as xo

N, C, H, W = 2, 5, 5, 7
NAMES = ('fp16', 'bf16')


@pytest.fixture
def calls(oracle_native, monkeypatch):
    """The three bindings replaced by the oracles' stand-ins, each call recorded: (binding, dtypes of the two feature tensors)"""
    from oflibpytorch_amd import _matching
    log = []

    def spy(name, fake):
        def run(feat, other, *args, **kw):
            log.append((name, feat.dtype, other.dtype))
            return fake(feat, other, *args, **kw)
        return run
    monkeypatch.setattr(_matching, "flow_global_match", spy("f32", mo.fake_flow_global_match))
    monkeypatch.setattr(_matching, "flow_global_match_x16", spy("x16", xo.fake_flow_global_match_x16))
    monkeypatch.setattr(_matching, "flow_global_match_grad", spy("grad", mo.fake_flow_global_match_grad))
    return log


@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("name", NAMES)
def test_a_matched_16_bit_pair_is_accepted_and_takes_the_new_binding(calls, name, ref):
    import oflibpytorch_amd as ofl
    dtype = xo.DTYPES[name]
    f16, o16, fup, oup = xo.features_general(name, N, C, H, W)
    want = mo.compute(fup, oup, -1.0 if ref == 's' else 1.0)
    res = ofl.Flow.from_matching(f16, o16, ref, return_prob=True)
    assert calls == [("x16", dtype, dtype)]
    flow, prob = res
    assert isinstance(flow, ofl.Flow) and flow.ref == ref and flow.shape == (N, H, W)
    assert flow.vecs.dtype == torch.float32 and not flow.vecs.requires_grad and np.array_equal(flow.vecs.numpy(), want['out32'])
    assert prob.dtype == torch.float32 and prob.shape == (N, H, W) and np.array_equal(prob.numpy(), want['prob'])
    one = ofl.Flow.from_matching(f16[1], o16[1], ref)                                        # C-H-W: a batch of one
    assert one.shape == (1, H, W) and np.array_equal(one.vecs.numpy()[0], want['out32'][1])
    got, prob = ofl.global_matching_flow(f16[0], o16[0], ref, return_prob=True)
    assert got.dtype == torch.float32 and got.shape == (2, H, W) and prob.shape == (H, W)
    assert [c[0] for c in calls] == ["x16"] * 3


def test_float32_features_take_the_old_binding(calls):
    import oflibpytorch_amd as ofl
    feat, other = (torch.from_numpy(a.copy()) for a in mo.features_general(N, C, H, W))
    ofl.Flow.from_matching(feat, other, 's')
    f = feat.clone().requires_grad_(True)
    ofl.Flow.from_matching(f, other, 's').vecs.backward(torch.from_numpy(mo.upstream(N, H, W).copy()))
    assert calls == [("f32", torch.float32, torch.float32)] * 2 + [("grad", torch.float32, torch.float32)]
    assert f.grad.dtype == torch.float32


@pytest.mark.parametrize("need", ["feat", "other", "both"])
@pytest.mark.parametrize("name", NAMES)
def test_gradients_come_in_the_features_dtype_and_nothing_float32_is_saved(calls, name, need):
    import oflibpytorch_amd as ofl
    dtype = xo.DTYPES[name]
    f16, o16, fup, oup = xo.features_general(name, N, C, H, W)
    g = mo.upstream(N, H, W)
    ft = f16.clone().requires_grad_(need in ("feat", "both"))
    ot = o16.clone().requires_grad_(need in ("other", "both"))
    flow, prob = ofl.Flow.from_matching(ft, ot, 's', return_prob=True)
    fn = flow.vecs.grad_fn
    assert type(fn).__name__ == "GlobalMatchFnBackward" and not prob.requires_grad
    saved = fn.saved_tensors
    assert [t.dtype for t in saved] == [dtype, dtype, torch.uint8]                           # the two features and the statistics
    assert saved[0].data_ptr() == ft.data_ptr() and saved[1].data_ptr() == ot.data_ptr()     # the tensors themselves, no copy
    flow.vecs.backward(torch.from_numpy(g.copy()))
    assert calls == [("x16", dtype, dtype), ("grad", torch.float32, torch.float32)]          # the up-conversions live in the backward only
    want = mo.grads(fup, oup, -1.0, g)
    for t, key, wanted in ((ft, 'd_feat', need in ("feat", "both")), (ot, 'd_other', need in ("other", "both"))):
        if wanted:
            assert t.grad.dtype == dtype and t.grad.shape == t.shape
            assert torch.equal(t.grad, torch.from_numpy(want[key]).to(dtype))                # rounded once
        else:
            assert t.grad is None
    # a C-H-W operand gets a C-H-W gradient
    f3 = f16[0].clone().requires_grad_(True)
    ofl.Flow.from_matching(f3, o16[0], 's').vecs.backward(torch.from_numpy(g[:1].copy()))
    assert f3.grad.shape == (C, H, W) and f3.grad.dtype == dtype
    assert torch.equal(f3.grad, torch.from_numpy(mo.grads(fup[:1], oup[:1], -1.0, g[:1])['d_feat'][0]).to(dtype))


def test_mixed_pairs_and_other_dtypes_are_refused_with_the_pinned_messages(oracle_native, monkeypatch):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _matching

    def never(*args, **kw):
        raise AssertionError("the checks come before the kernel")
    good = torch.zeros(2, 3, 5, 7)
    with pytest.raises(TypeError, match="float16 or bfloat16"):                              # the binding checks for itself
        _matching.flow_global_match_x16(good, good)
    for name in ("flow_global_match", "flow_global_match_x16", "flow_global_match_grad"):
        monkeypatch.setattr(_matching, name, never)
    pairs = [(good.half(), good), (good, good.half()), (good.bfloat16(), good), (good, good.bfloat16()), (good.half(), good.bfloat16()),
             (good.bfloat16(), good.half()), (good.double(), good.double()), (good.to(torch.uint8), good.to(torch.uint8)),
             (good.half(), good.double())]
    for a, b in pairs:
        with pytest.raises(TypeError, match=r"^Error matching flow: .*float32"):
            ofl.Flow.from_matching(a, b)
        with pytest.raises(TypeError, match=r"^Error matching flow: "):
            ofl.global_matching_flow(a, b, 's')
        with pytest.raises(TypeError, match="float32"):
            _matching.check_features(a, b)
        with pytest.raises(TypeError, match="float32"):
            _matching.global_match(a, b)
    for a in (good, good.half(), good.bfloat16()):
        _matching.check_features(a, a)                                                       # the three matched pairs pass
    with pytest.raises(ValueError, match="same shape"):
        _matching.check_features(good.half(), good.half()[:1])
    assert _matching.X16 == {torch.float16: 0, torch.bfloat16: 1}


def test_the_docstrings_say_what_16_bit_features_get():
    import oflibpytorch_amd as ofl
    for doc in (ofl.Flow.from_matching.__doc__, ofl.global_matching_flow.__doc__, ofl.__doc__):
        doc = " ".join(doc.split())
        assert "bfloat16" in doc and "float16" in doc and "3.32" in doc


# ---- the oracle module's own claims ---------------------------------------------------------------------------------------------------
def test_geometry_frames_and_channels():
    g = xo.geometry()
    assert g == dict(kTileP=64, kSubP=32, kChunkQ=32, kLaneQ=16, kKStep=16, kRegSteps=8, kQPad=64)
    assert sorted(f[1] * f[2] for f in xo.frames()) == [1, 5, 5, 31, 32, 33, 35, 63, 64, 65, 129]
    assert (1, 1, 5) in xo.frames() and (1, 5, 1) in xo.frames() and (3, 5, 7) in xo.frames()
    assert xo.channels() == [1, 15, 16, 17, 31, 32, 33, 128, 130]


@pytest.mark.parametrize("name", NAMES)
def test_the_general_features_are_exact_in_the_dtype_but_for_the_named_elements(name):
    """Multiples of 2^-6: float16 holds every one of them; bfloat16 all below 4 in magnitude and, above, those whose odd part fits 8 bits.
    The count the cast changes is printed and asserted element by element inside xo.features_general"""
    changed = total = 0
    for shape in ((3, 5, 5, 7), (1, 130, 3, 43), (1, 24, 11, 97)):
        a, b = mo.features_general(*shape)
        _, _, fup, oup = xo.features_general(name, *shape)
        for raw, up in ((a, fup), (b, oup)):
            changed += int((raw != up).sum())
            total += raw.size
            assert (np.abs(raw)[raw != up] >= 4).all()
    print("%s: the cast changes %d of %d elements" % (name, changed, total))
    assert changed == 0 if name == 'fp16' else changed < total // 1000
    assert xo.bf16_changes(np.array([4.015625, 4.03125, 3.984375, 8.03125, 8.0625, 0.0])).tolist() == [True, False, False, True, False, False]


@pytest.mark.parametrize("c", [4, 16])
def test_the_exact_families_on_the_new_borders_are_what_they_say(c):
    g = xo.geometry()
    n, h, w = 3, 5, 13                                                                       # Q = 65: a tile and two chunks, plus one
    q = h * w
    for kind in ('one-hot', 'two-hot', 'all-equal') + (('rising',) if c == 16 else ()):
        feat, other = xo.features_exact(kind, n, c, h, w)
        assert set(np.unique(feat).tolist()) <= {0.0, 32.0} and set(np.unique(other).tolist()) <= {0.0, -32.0}
        for dtype in xo.DTYPES.values():
            assert np.array_equal(xo.to16(feat, dtype)[1], feat) and np.array_equal(xo.to16(other, dtype)[1], other)
        r = mo.compute(feat, other, -1.0)
        wide = mo.compute(feat, other, -1.0, wide=True)
        assert ((r['s'] == 0) | (r['s'] <= -1024)).all() and np.array_equal(r['out'], wide['out']) and np.array_equal(r['S'], wide['S'])
        wt = r['w']
        if kind == 'one-hot':
            tg = xo.targets(kind, q, c)
            assert set(np.unique(wt).tolist()) == {0.0, 1.0} and q - 1 in tg
            assert c == 4 or {0, 3, 4, g["kChunkQ"] - 1, g["kChunkQ"], g["kTileP"] - 1, g["kTileP"]} <= set(tg)
            assert set(np.unique(wt.argmax(2)).tolist()) == set(tg)                           # every named position is somebody's match
        elif kind == 'two-hot':
            assert set(np.unique(wt).tolist()) == {0.0, 0.5}
            first, second = wt.argmax(2), q - 1 - wt[:, :, ::-1].argmax(2)
            assert (first // g["kChunkQ"] != second // g["kChunkQ"]).all()
            assert ((first % 8 < 4) != (second % 8 < 4)).all()                               # ... and in the other half of the lanes
        elif kind == 'all-equal':
            assert np.array_equal(r['S'], np.full((n, q), float(q)))
        else:
            assert np.array_equal(r['m'], np.zeros((n, q), np.float32)) and set(np.unique(wt).tolist()) == {0.0, 1.0}


@pytest.mark.parametrize("name", NAMES)
def test_mutants_miss_by_far_and_padding_counted_as_zero_fails_the_bar_at_every_tail(name):
    """The four mutants of matching_oracle each miss the textbook expression by more than a tenth of the result's scale, as in 3.27, on the
    16-bit values.  The new one -- the padded positions of the last chunk counted with a logit of 0 -- must fail the forward's bar at
    every frame of the GPU tier whose Q is no multiple of the chunk, and IS the definition where it is one"""
    _, _, fup, oup = xo.features_general(name, N, C, H, W)
    want = mo.textbook(fup, oup, 1.0)['out']
    scale = np.abs(want).max()
    assert np.abs(xo.compute(fup, oup, 1.0)['out'] - want).max() <= 1e-12 * scale
    for mutant in mo.MUTANTS:
        miss = np.abs(xo.compute(fup, oup, 1.0, mutant=mutant)['out'] - want).max()
        print("%s %s: misses by %.3f of the scale" % (name, mutant, miss / scale))
        assert miss > 0.1 * scale
    chunk = xo.geometry()["kChunkQ"]
    tails = 0
    for n, h, w in xo.frames():
        _, _, fup, oup = xo.features_general(name, n, 16, h, w)
        good = xo.compute(fup, oup, -1.0)
        frac = (np.abs(xo.compute(fup, oup, -1.0, mutant='padded_zero')['out'] - good['out']) / good['bar']).max()
        print("%s %d x %d x %d: padding counted as 0 is at %.3g of the bar" % (name, n, h, w, frac))
        if (h * w) % chunk:
            tails += 1
            assert frac > 1.0
        else:
            assert frac == 0.0
    assert tails >= 8


def test_a_t_flow_is_the_exact_negation_of_an_s_flow_with_the_same_bars():
    """What lets the GPU tier evaluate the oracle once per case: the sign enters as a factor of -1 alone"""
    _, _, fup, oup = xo.features_general('bf16', N, C, H, W)
    g = mo.upstream(N, H, W)
    s, t = xo.compute(fup, oup, -1.0), xo.compute(fup, oup, 1.0)
    assert np.array_equal(t['out'], -s['out']) and np.array_equal(t['bar'], s['bar']) and np.array_equal(t['bar_prob'], s['bar_prob'])
    assert np.array_equal(t['ox'], s['ox']) and np.array_equal(t['loose'], s['loose'])
    gs, gt = xo.grads(fup, oup, -1.0, g, 'bf16', s), xo.grads(fup, oup, 1.0, g, 'bf16', t)
    for key in ('feat', 'other'):
        assert np.array_equal(gt['d_' + key], -gs['d_' + key]) and np.array_equal(gt['bar_' + key], gs['bar_' + key])
        half = xo.rounded_to(gs, 'fp16')
        assert np.array_equal(half['bar32_' + key], gs['bar32_' + key]) and (half['bar_' + key] <= gs['bar_' + key]).all()


def test_the_bars_are_small_and_made_of_the_named_terms():
    """C = 16, 5 x 13: eta is the accumulation's, the exponential's and the chunk sum's terms; the bar stays far below the flow's scale"""
    _, _, fup, oup = xo.features_general('bf16', 1, 16, 5, 13)
    r = xo.compute(fup, oup, -1.0)
    u = 2.0 ** -24
    assert (r['eta'] >= (2 + 15) * u).all() and (r['eta'] <= (18 * r['absdot'].max() + 2 + 3 * 104 + 15 + 1) * u).all()
    assert r['bar'].max() < 1e-3 and np.abs(r['out']).max() > 1
    assert (r['A'] >= 0).all() and (r['B'] >= 0).all() and (r['B'] <= 12).all()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_c_abi_declarations_and_argument_checks_need_no_gpu():
    from oflibpytorch_amd import _matching, _native
    names = {"ofl_flow_global_match_x16", "ofl_flow_global_match_x16_pack_bytes"}
    assert names <= set(_native.exported_symbols())
    header = open(_native._build.HEADERS[0]).read()
    for name in names:
        assert (" %s(" % name) in header
    assert any(src.endswith("ofl_matching_x16.hip") for src in _native._build.SOURCES)
    lib = _matching._library()
    assert lib.ofl_version() == _native.ABI_VERSION == 36                # names were added, no signature changed
    pack = lib.ofl_flow_global_match_x16_pack_bytes
    assert pack(1, 1, 1, 1) == 2 * 64 * 16 * 2 and pack(16, 3, 5, 7) == 2 * 3 * 64 * 16 * 2 and pack(17, 1, 5, 13) == 2 * 128 * 32 * 2
    assert pack(130, 8, 135, 240) == 2 * 8 * 32448 * 144 * 2
    for bad in ((0, 1, 4, 4), (4, 0, 4, 4), (4, 1, 0, 4), (4, 1, 4, 0), (4, 65536, 4, 4), (4, 1, 65536, 32768), (4, 1, (1 << 24) + 1, 1)):
        assert pack(*bad) == -3, bad
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(4096)               # never dereferenced: every call below is rejected first
    odd, odd4, odd8 = ctypes.c_void_p(4097), ctypes.c_void_p(4098), ctypes.c_void_p(4104)

    def fwd(feat=one, feat_bs=0, other=one, other_bs=0, c=4, elem=0, sign=-1.0, out=one, prob=one, stats=one, ws=one, n=1, h=4, w=4):
        return lib.ofl_flow_global_match_x16(feat, feat_bs, other, other_bs, c, elem, sign, out, prob, stats, ws, n, h, w, null)
    for kw in (dict(n=0), dict(n=65536), dict(n=-3), dict(h=0), dict(w=0), dict(h=-1), dict(c=0), dict(c=-2), dict(sign=0.0), dict(sign=2.0),
               dict(h=65536, w=32768), dict(h=(1 << 24) + 1, w=1), dict(h=1, w=(1 << 24) + 1), dict(elem=2), dict(elem=-1),
               dict(feat=null), dict(other=null), dict(out=null), dict(ws=null), dict(feat_bs=-1), dict(other_bs=-1),
               dict(feat=odd), dict(other=odd), dict(out=odd4), dict(prob=odd4), dict(stats=odd4), dict(ws=odd8)):
        assert fwd(**kw) == -3, kw
