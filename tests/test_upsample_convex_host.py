"""CPU tier of Flow.upsample_convex: the oracle (tests/upsample_convex_oracle.py) against RAFT's own expression in torch
float64 and its autograd, three mutants that the comparison must tell apart, the exact-softmax inputs of the GPU tier, the host logic of
the API with the native calls served by the oracle, every argument check that needs no device, and the C ABI's declarations and argument
checks.  No device."""
import ctypes

import numpy as np
import pytest
import torch

import upsample_convex_oracle as uo

N, H, W = 2, 5, 7


@pytest.fixture
def up_native(oracle_native, monkeypatch):
    from oflibpytorch_amd import _upsample
    monkeypatch.setattr(_upsample, "flow_upsample_convex", uo.fake_flow_upsample_convex)
    monkeypatch.setattr(_upsample, "flow_upsample_convex_grad", uo.fake_flow_upsample_convex_grad)
    return _upsample


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x).copy())


def _flow(ref='t', n=N, h=H, w=W, masked=True):
    import oflibpytorch_amd as ofl
    f, m = uo.case(n, h, w)
    return ofl.Flow(_t(f), ref, _t(m) if masked else None)


# ---- the oracle computes RAFT's expression --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", uo.FACTORS)
def test_float64_evaluation_is_rafts_expression_and_its_autograd(k):
    """5 x 7, a batch of 2: the oracle's float64 evaluation, and its gradients, against RAFT's expression in torch float64 and torch's
    autograd of it, within 1e-12 of each result's scale (under 600 float64 roundings of 1.1e-16 on terms of that scale)."""
    f, _ = uo.case(N, H, W)
    lg, g = uo.logits_general(N, k, H, W), uo.upstream(N, k, H, W)
    want = uo.raft_reference(f, lg, k, g)
    got = uo.compute(f, lg, k, float64=True)['out']
    gr = uo.grads(f, lg, k, g, float64=True)
    for name, a, b in (("out", got, want['out']), ("d logits", gr['d_logits'], want['d_logits']), ("d flow", gr['d_flow'], want['d_flow'])):
        scale = np.abs(b).max()
        err = np.abs(a - b).max()
        print("k %d %s: largest |oracle float64 - RAFT float64| = %.3e of a scale %.3e" % (k, name, err, scale))
        assert a.dtype == np.float64 and a.shape == b.shape and scale > 1.0
        assert err <= 1e-12 * scale, name
    # the float32 results are those values rounded once
    assert np.array_equal(uo.compute(f, lg, k)['out'], got.astype(np.float32))
    g32 = uo.grads(f, lg, k, g)
    assert np.array_equal(g32['d_logits'], gr['d_logits'].astype(np.float32)) and np.array_equal(g32['d_flow'], gr['d_flow'].astype(np.float32))


@pytest.mark.parametrize("mutant", ["swap_ij", "dx_outer", "over_k2"])
@pytest.mark.parametrize("k", uo.FACTORS)
def test_mutants_fail_the_comparison(k, mutant):
    """A swapped i / j, a tap order with dx outermost and weights normalised over k^2 instead of the nine taps each miss RAFT's expression
    by far more than the bar, on the same inputs"""
    f, _ = uo.case(N, H, W)
    lg = uo.logits_general(N, k, H, W)
    want = uo.raft_reference(f, lg, k)['out']
    got = uo.compute(f, lg, k, float64=True, **{mutant: True})['out']
    scale = np.abs(want).max()
    assert np.abs(got - want).max() > 1e-3 * scale
    assert np.abs(uo.compute(f, lg, k, float64=True)['out'] - want).max() <= 1e-12 * scale


@pytest.mark.parametrize("k", uo.FACTORS)
def test_the_exact_inputs_are_what_they_say(k):
    """The bit-for-bit tier of the GPU tests rests on these: every weight is 1 / 9, 1 or 0, or 1 / 2 or 0, and the one-hot output is k times
    the named neighbour, zeros at the border"""
    n, h, w = 3, 5, 7
    f, _ = uo.case(n, h, w)
    wt = uo.weights(uo.logits_exact('constant', n, k, h, w), k)[0]
    assert np.array_equal(wt, np.full_like(wt, 1.0 / 9.0))
    assert set(np.unique(uo.logits_exact('constant', n, k, h, w)).tolist()) == {0.0, 3.5, -87.0}
    wt = uo.weights(uo.logits_exact('one-hot', n, k, h, w), k)[0]
    assert set(np.unique(wt).tolist()) == {0.0, 1.0} and np.array_equal(wt.sum(1), np.ones_like(wt[:, 0]))
    hot = uo.hot_tap(n, k, h, w)
    assert np.array_equal(wt.argmax(1), hot) and len(np.unique(hot)) == 9
    nb = uo.neighbours(f, k)
    want = np.take_along_axis(nb[:, :, :, None, None], np.broadcast_to(hot[:, None, None], (n, 2, 1, k, k, h, w)), 2)[:, :, 0]
    out = uo.compute(f, uo.logits_exact('one-hot', n, k, h, w), k)['out']
    assert np.array_equal(out, uo._fine(want, k).astype(np.float32))
    border = hot[:, :, :, 0, 0] == 0                                                          # tap (-1, -1) of the corner pixel: outside
    assert border.any() and not uo._fine(want, k)[:, :, :k, :k][np.broadcast_to(border[:, None], (n, 2, k, k))].any()
    wt = uo.weights(uo.logits_exact('two-hot', n, k, h, w), k)[0]
    assert set(np.unique(wt).tolist()) == {0.0, 0.5} and np.array_equal((wt == 0.5).sum(1), np.full(wt[:, 0].shape, 2))


def test_non_finite_values_follow_ieee():
    k, n, h, w = 2, 1, 3, 4
    f, _ = uo.case(n, h, w)
    base = uo.logits_general(n, k, h, w)
    clean = uo.compute(f, base, k)['out']
    for name, edit in (("nan", lambda a: a.__setitem__((0, 1 * 4 + 1 * 2 + 0, 1, 2), np.nan)),
                       ("+inf", lambda a: a.__setitem__((0, 4 * 4 + 1 * 2 + 0, 1, 2), np.inf)),
                       ("all -inf", lambda a: a.__setitem__((0, slice(2, None, 4), 1, 2), -np.inf))):
        lg = base.copy()
        edit(lg)
        out = uo.compute(f, lg, k)['out']
        bad = np.zeros_like(out, bool)
        bad[:, :, 2 * 1 + 1, 2 * 2 + 0] = True                                                # i = 1, j = 0 of coarse pixel (1, 2)
        assert np.isnan(out[bad]).all() and np.array_equal(out[~bad], clean[~bad]), name
    lg = base.copy()
    lg[0, 3 * 4 + 1 * 2 + 1, 1, 2] = -np.inf                                                  # a weight of exactly 0: everything stays finite
    out = uo.compute(f, lg, k)['out']
    assert np.isfinite(out).all() and uo.weights(lg, k)[0][0, 3, 1, 1, 1, 2] == 0.0
    fi = f.copy()
    fi[0, 0, 0, 0] = np.inf                                                                   # a corner vector: 4 coarse pixels, channel 0
    out = uo.compute(fi, base, k)['out']
    bad = np.zeros_like(out, bool)
    bad[0, 0, :4, :4] = True
    assert (~np.isfinite(out[bad])).all() and np.array_equal(out[~bad], clean[~bad])


# ---- the host logic of the API, the oracle in the bindings' place ---------------------------------------------------------------------
@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("k", uo.FACTORS)
def test_shapes_values_mask_and_ref(up_native, ref, k):
    import oflibpytorch_amd as ofl
    f, m = uo.case(N, H, W)
    lg = uo.logits_general(N, k, H, W)
    flow = _flow(ref)
    up = flow.upsample_convex(_t(lg))                                                          # the factor is inferred
    assert isinstance(up, ofl.Flow) and up.ref == ref and up.shape == (N, k * H, k * W) and up.device == flow.device
    assert up.vecs.dtype == torch.float32 and not up.vecs.requires_grad
    assert np.array_equal(up.vecs.numpy(), uo.compute(f, lg, k)['out'])
    assert np.array_equal(up.mask.numpy(), uo.mask_of(m, k))
    assert torch.equal(up.mask, flow.mask.repeat_interleave(k, 1).repeat_interleave(k, 2))
    same = flow.upsample_convex(lg.copy(), factor=k, consider_mask=True)                       # arrays are taken
    assert np.array_equal(same.vecs.numpy(), up.vecs.numpy()) and torch.equal(same.mask, up.mask)
    bare = flow.upsample_convex(_t(lg), consider_mask=False)
    assert bool(bare.mask.all()) and np.array_equal(bare.vecs.numpy(), up.vecs.numpy())        # the mask does not enter the arithmetic
    # [9 k^2, H, W] weights for a batch of 1, and the tensor wrapper
    one = ofl.Flow(_t(f[1:]), ref, _t(m[1:])).upsample_convex(_t(lg[1]))
    assert one.shape == (1, k * H, k * W) and np.array_equal(one.vecs.numpy()[0], up.vecs.numpy()[1])
    got = ofl.upsample_flow_convex(_t(f[1]), _t(lg[1]))
    assert got.shape == (2, k * H, k * W) and np.array_equal(got.numpy(), up.vecs.numpy()[1])
    got = ofl.upsample_flow_convex(f.copy(), lg.copy(), factor=k)
    assert got.shape == (N, 2, k * H, k * W) and np.array_equal(got.numpy(), up.vecs.numpy())


@pytest.mark.parametrize("need", ["none", "logits", "vecs", "both"])
def test_requires_grad_routing(up_native, monkeypatch, need):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _autograd
    k = 4
    f, m = uo.case(N, H, W)
    lg, g = uo.logits_general(N, k, H, W), uo.upstream(N, k, H, W)
    calls = []
    real = uo.fake_flow_upsample_convex_grad

    def spy(vecs, logits, factor, grad_out, want_logits=True, want_vecs=True):
        calls.append((want_logits, want_vecs))
        return real(vecs, logits, factor, grad_out, want_logits, want_vecs)
    monkeypatch.setattr(up_native, "flow_upsample_convex_grad", spy)
    v = _t(f).requires_grad_(need in ("vecs", "both"))
    lt = _t(lg).requires_grad_(need in ("logits", "both"))
    up = ofl.Flow(v, 's', _t(m)).upsample_convex(lt)
    assert issubclass(_autograd.UpsampleConvexFn, torch.autograd.Function)
    if need == "none":
        assert not up.vecs.requires_grad and up.vecs.grad_fn is None
        return
    assert up.vecs.requires_grad and type(up.vecs.grad_fn).__name__ == "UpsampleConvexFnBackward"
    assert not up.mask.requires_grad and up.mask.dtype == torch.bool
    up.vecs.backward(_t(g))
    assert calls == [(need in ("logits", "both"), need in ("vecs", "both"))]
    want = uo.grads(f, lg, k, g)
    if need in ("logits", "both"):
        assert lt.grad.dtype == torch.float32 and np.array_equal(lt.grad.numpy(), want['d_logits'])
    else:
        assert lt.grad is None
    if need in ("vecs", "both"):
        assert v.grad.dtype == torch.float32 and np.array_equal(v.grad.numpy(), want['d_flow'])
    else:
        assert v.grad is None
    with torch.no_grad():
        assert not ofl.Flow(v, 's').upsample_convex(lt).vecs.requires_grad


def test_api_checks_and_their_messages(oracle_native, monkeypatch):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _upsample

    def never(*args, **kw):
        raise AssertionError("the checks come before the kernel")
    monkeypatch.setattr(_upsample, "flow_upsample_convex", never)
    monkeypatch.setattr(_upsample, "upsample_convex", never)
    flow = _flow()
    pre = r"Error upsampling flow: "
    good = torch.zeros(N, 36, H, W)
    call = flow.upsample_convex
    for bad in ("weights", 3, None, [good]):
        with pytest.raises(TypeError, match=pre + "Weights need to be a torch tensor or a numpy array"):
            call(bad)
    for bad in (good.double(), good.half(), good.bfloat16(), good.to(torch.uint8), np.zeros((N, 36, H, W))):
        with pytest.raises(TypeError, match=pre + "Weights need to be of dtype float32"):
            call(bad)
    for bad in (torch.zeros(H, W), torch.zeros(1, N, 36, H, W)):
        with pytest.raises(ValueError, match=pre + "Weights need to have 3 or 4 dimensions"):
            call(bad)
    for c in (0, 9, 35, 37, 81, 9 * 9, 9 * 256):
        with pytest.raises(ValueError, match=pre + "Weights need to have 9 k\\^2 channels with k 2, 4 or 8"):
            call(torch.zeros(N, c, H, W))
    for bad in (True, 2.0, "2", [2]):
        with pytest.raises(TypeError, match=pre + "Factor needs to be an integer"):
            call(good, factor=bad)
    for bad in (0, 1, 3, 16, -2):
        with pytest.raises(ValueError, match=pre + "Factor needs to be 2, 4 or 8"):
            call(good, factor=bad)
    for bad in (4, 8):
        with pytest.raises(ValueError, match=pre + "Factor %d contradicts the 36 channels" % bad):
            call(good, factor=bad)
    for bad in (torch.zeros(1, 36, H, W), torch.zeros(3, 36, H, W), torch.zeros(36, H, W)):
        with pytest.raises(ValueError, match=pre + "Weights need to have the batch size of the flow"):
            call(bad)
    for bad in (torch.zeros(N, 36, W, H), torch.zeros(N, 36, H, W + 1), torch.zeros(N, 36, 2 * H, 2 * W)):
        with pytest.raises(ValueError, match=pre + "Weights need to have the H-W shape of the flow"):
            call(bad)
    for bad in (1, 0, "True"):
        with pytest.raises(TypeError, match=pre + "Consider_mask needs to be boolean"):
            call(good, consider_mask=bad)
    with pytest.raises(ValueError, match=pre):
        ofl.upsample_flow_convex(flow.vecs, good, factor=4)
    with pytest.raises(TypeError, match=pre):
        ofl.upsample_flow_convex(flow.vecs, good.double())
    # the bindings check for themselves
    with pytest.raises(ValueError, match="not 9 k\\^2"):
        _upsample.factor_of(81)
    assert [_upsample.factor_of(9 * k * k) for k in (2, 4, 8)] == [2, 4, 8] == [uo.factor_of(9 * k * k) for k in (2, 4, 8)]
    with pytest.raises(ValueError, match="at least one output"):
        _upsample.flow_upsample_convex_grad(flow.vecs, good, 2, torch.zeros(N, 2, 2 * H, 2 * W), want_logits=False, want_vecs=False)


def test_the_method_and_the_wrapper_are_exported():
    import oflibpytorch_amd as ofl
    assert callable(ofl.Flow.upsample_convex) and callable(ofl.upsample_flow_convex)
    doc = " ".join(ofl.Flow.upsample_convex.__doc__.split())
    assert "RAFT's channel order" in doc and "not with respect to the mask" in doc
    assert "upsample_convex" in ofl.__doc__


# ---- the C ABI: declared, exported, and every rejected argument is rejected before any launch -----------------------------------------
def test_c_abi_declarations_and_argument_checks_need_no_gpu():
    from oflibpytorch_amd import _native, _upsample
    names = {"ofl_flow_upsample_convex_f32", "ofl_flow_upsample_convex_grad_f32"}
    assert names <= set(_native.exported_symbols())
    header = open(_native._build.HEADERS[0]).read()
    for name in names:
        assert (" %s(" % name) in header
    assert _upsample.FACTORS == uo.FACTORS == (2, 4, 8)
    assert any(src.endswith("ofl_upsample.hip") for src in _native._build.SOURCES)
    lib = _upsample._library()
    assert lib.ofl_version() == _native.ABI_VERSION == 36                # names were added, no signature changed
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(4096)               # never dereferenced: every call below is rejected first
    odd, odd8, odd16 = ctypes.c_void_p(4098), ctypes.c_void_p(4100), ctypes.c_void_p(4104)

    def fwd(flow=one, flow_bs=0, half=0, mask=one, mask_bs=0, logits=one, factor=2, out=one, out_mask=one, n=1, h=4, w=4):
        return lib.ofl_flow_upsample_convex_f32(flow, flow_bs, half, mask, mask_bs, logits, factor, out, out_mask, n, h, w, null)

    def bwd(flow=one, flow_bs=0, half=0, logits=one, factor=2, g=one, dl=one, df=one, ws=one, n=1, h=4, w=4):
        return lib.ofl_flow_upsample_convex_grad_f32(flow, flow_bs, half, logits, factor, g, dl, df, ws, n, h, w, null)
    frame = (dict(n=0), dict(n=65536), dict(n=-3), dict(h=0), dict(w=0), dict(h=-1), dict(factor=0), dict(factor=1), dict(factor=3),
             dict(factor=16), dict(factor=-2),
             dict(h=32768, w=32768, factor=2),          # the coarse frame passes (2^30 pixels), the fine grid does not (2^32)
             dict(h=16384, w=16384, factor=8), dict(h=1, w=1 << 30, factor=2), dict(h=1 << 29, w=1, factor=8),
             dict(flow=null), dict(logits=null), dict(flow_bs=-1), dict(half=2), dict(half=-1), dict(flow=odd),
             dict(flow=ctypes.c_void_p(4097), half=1), dict(logits=odd))
    for kw in frame + (dict(out=null), dict(mask_bs=-1), dict(mask=null), dict(out_mask=null), dict(out=odd8), dict(out=odd16),
                       dict(out_mask=odd8)):
        assert fwd(**kw) == -3, kw
    for kw in frame + (dict(g=null), dict(dl=null, df=null, ws=null), dict(ws=null), dict(df=null), dict(g=odd16), dict(dl=odd), dict(df=odd),
                       dict(ws=odd8)):
        assert bwd(**kw) == -3, kw
