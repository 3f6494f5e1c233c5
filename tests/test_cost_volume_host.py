"""CPU tier of Flow.cost_volume: the oracle (tests/cost_volume_oracle.py) against the expression people mean
(`torch.nn.functional.unfold` of the masked warped tensor), its float32 order against its float64 evaluation within the derived bound,
its gradients against torch's float64 autograd of the written-out definition, the coverage condition of the GPU tier's inputs, the host
logic of the API with the native calls served by the oracle, every argument check that needs no device, and the C ABI's declarations
and argument checks.  No device."""
import ctypes

import numpy as np
import pytest
import torch

import cost_volume_oracle as cv
import grad_oracle64 as go
import photometric_oracle as po

# the frames of the GPU tier (tests/test_gpu_cost_volume.py): 20 x 28, the kernel's tile minus one, itself, plus one, two tiles plus one
# in both axes, a frame smaller than the window, a batch of 3
GPU_FRAMES = cv.frames()


@pytest.fixture
def cv_native(oracle_native, monkeypatch):
    from oflibpytorch_amd import _cost_volume
    monkeypatch.setattr(_cost_volume, "flow_cost_volume", cv.fake_flow_cost_volume)
    monkeypatch.setattr(_cost_volume, "flow_cost_volume_grad", cv.fake_flow_cost_volume_grad)
    monkeypatch.setattr(_cost_volume, "flow_cost_volume_chain", cv.fake_flow_cost_volume_chain)
    monkeypatch.setattr(_cost_volume, "flow_cost_volume_gate", cv.fake_flow_cost_volume_gate)
    return _cost_volume


# ---- the oracle computes the expression people mean ----------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", cv.RADII)
def test_float64_evaluation_is_the_unfolded_correlation(radius):
    """unfold with zero padding of the masked warped tensor, times feat, mean over the channels, in torch float64 on the oracle's own
    W', against the oracle's float64 evaluation on an unmasked zero-flow frame: within 1e-12."""
    n, c, h, w = 2, 5, 20, 28
    a = np.zeros((n, 2, h, w), np.float32)
    worst = 0.0
    for ref in cv.REFS:
        feat, other = cv.features(n, c, h, w, ref)
        res = cv.compute(a, None, feat, other, ref, radius, float64=True)
        assert res['volume'].dtype == np.float64 and res['usable'].all()
        assert np.abs(res['warped'] - other).max() < 1e-4                                     # (the positions round: not bit for bit)
        win = 2 * radius + 1
        unf = torch.nn.functional.unfold(torch.from_numpy(res['warped'].copy()).double(), win, padding=radius)
        unf = unf.reshape(n, c, win * win, h, w)
        want = (torch.from_numpy(feat.copy()).double()[:, :, None] * unf).sum(1) / c
        worst = max(worst, float(np.abs(res['volume'] - want.numpy()).max()))
        assert np.abs(want.numpy()).max() > 0.1
    print("radius %d: largest |oracle float64 - unfolded correlation| = %.3e" % (radius, worst))
    assert worst <= 1e-12


def test_float32_definition_against_its_float64_evaluation():
    """C products, C sums from +0 and one division, each rounded once: the float32 volume is within (C + 2) 2^-24 (sum_c |feat W'|) / C
    of the float64 evaluation of the same steps, per entry."""
    worst = 0.0
    for (n, h, w), c in zip(GPU_FRAMES, (3, 16, 1, 35, 17, 4, 15)):
        for ref in cv.REFS:
            a, m = cv.case(n, h, w, ref)
            feat, other = cv.features(n, c, h, w, ref)
            for radius in (1, 4):
                r32, r64 = cv.compute(a, m, feat, other, ref, radius), cv.compute(a, m, feat, other, ref, radius, float64=True)
                assert r32['volume'].dtype == np.float32 and r32['volume'].shape == (n, (2 * radius + 1) ** 2, h, w)
                bound = (c + 2) * 2.0 ** -24 * r64['abs']
                err = np.abs(r32['volume'].astype(np.float64) - r64['volume'])
                assert np.all(err <= bound), (n, h, w, ref, radius, float((err - bound).max()))
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print("largest |float32 volume - float64 evaluation| is %.3f of the bound" % worst)


# ---- the oracle's gradients are the derivative ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 4])
@pytest.mark.parametrize("ref", cv.REFS)
def test_oracle_gradients_are_the_float64_derivative(ref, radius):
    """A 9 x 17 frame (h - 1 and w - 1 powers of two) with vectors on a grid of 2^-6, |a| < 4: every float32 sample position is exact.
    Features on a grid of 2^-8, so that every float32 W' is exact too.  d feat and d W of the oracle (float32, o ascending) are then
    within (D + 2) 2^-24 of the sum of their terms' absolute values of torch's float64 autograd (one division, D products, D sums);
    d other and d flow, the float64 backward of the warp applied to torch's d W, are torch's own within 1e-12 of their scale."""
    n, c, h, w = 3, 3, 9, 17
    rng = np.random.RandomState(31 + radius)
    a = (rng.randint(-255, 256, (n, 2, h, w)) / 64.0).astype(np.float32)
    mask = rng.uniform(size=(n, h, w)) >= 0.2
    feat, other = ((rng.randint(-256, 256, (n, c, h, w)) / 256.0).astype(np.float32) for _ in range(2))
    d = (2 * radius + 1) ** 2
    g = cv.upstream(n, d, h, w)
    res = cv.compute(a, mask, feat, other, ref, radius)
    assert 0.2 < res['usable'].mean() < 0.8 and (~res['inside']).mean() > 0.1
    want = cv.torch_reference(a, res['usable'], feat, other, ref, radius, g)
    assert np.array_equal(res['warped'].astype(np.float64), want['warped'])                   # the float32 W' are exact
    assert np.abs(cv.compute(a, mask, feat, other, ref, radius, float64=True)['volume'] - want['volume']).max() <= 1e-12
    d_feat, d_w = cv.grads(a, mask, feat, other, ref, radius, g, res=res)
    assert d_feat.dtype == np.float32 and d_w.dtype == np.float32
    big_f, big_w = cv.grads(a, mask, np.abs(feat), other, ref, radius, np.abs(g), float64=True,
                            res={'warped': np.abs(res['warped']), 'usable': res['usable']})
    for name, got, ref64, big in (("d feat", d_feat, want['d_feat'], big_f), ("d W", d_w, want['d_warped'], big_w)):
        err = np.abs(got.astype(np.float64) - ref64)
        print("ref %s radius %d %s: max error %.3e of a scale %.3e" % (ref, radius, name, err.max(), np.abs(ref64).max()))
        assert np.abs(ref64).max() > 1e-2 and np.all(err <= (d + 2) * 2.0 ** -24 * big), name
    unusable = ~np.broadcast_to(res['usable'][:, None], d_w.shape)
    assert not d_w[unusable].view(np.uint32).any() and not want['d_warped'][unusable].any()   # exactly +0 where not usable
    d_other, d_flow = cv.chain(a, other, want['d_warped'], ref)
    for name, got, ref64 in (("d other", d_other, want['d_other']), ("d flow", d_flow, want['d_flow'])):
        scale = np.abs(ref64).max()
        assert scale > 1e-2 and np.abs(got - ref64).max() <= 1e-12 * scale, name
    assert not d_flow[~np.broadcast_to(res['usable'][:, None], d_flow.shape)].any()           # the `usable` gating reaches the flow


# ---- the coverage condition of the GPU tier's inputs ----------------------------------------------------------------------------------
def test_every_gpu_frame_of_9_by_9_and_larger_shows_every_category():
    """No GPU test can pass on an empty set.  Per image and for both refs, on every frame of the GPU tier of at least 9 x 9: at least
    20 % of the pixels are usable, 10 % sample outside the frame and 5 % are masked only."""
    checked = 0
    for n, h, w in GPU_FRAMES:
        if h < 9 or w < 9:
            continue
        for ref in cv.REFS:
            known, outside, masked = po.categories(n, h, w, ref)
            print("%d x %d x %d '%s': usable %s outside %s masked only %s" % (
                n, h, w, ref, *(np.round(100 * x, 1).tolist() for x in (known, outside, masked))))
            assert known.min() >= 0.2 and outside.min() >= 0.1 and masked.min() >= 0.05, (n, h, w, ref)
            a, m = cv.case(n, h, w, ref)
            _, usable, inside = cv.warped(a, m, cv.features(n, 2, h, w, ref)[1], ref)
            assert np.array_equal(usable.sum((1, 2)) / float(h * w), known) and np.array_equal((~inside).sum((1, 2)) / float(h * w), outside)
            checked += 1
    assert checked == 2 * (len(GPU_FRAMES) - 1)


def test_hand_computed_pixel():
    """Zero flow on a 2 x 2 frame, two channels, radius 1: entry o of pixel (0, 0) holds feat(0, 0) . other((0, 0) + o) / 2 where that
    pixel is in the frame and usable, +0 elsewhere."""
    f32 = np.float32
    a = np.zeros((1, 2, 2, 2), f32)
    mask = np.array([[[True, True], [True, False]]])
    feat = np.array([[[[0.5, 0.0], [0.0, 0.0]], [[-0.25, 0.0], [0.0, 0.0]]]], f32)
    other = np.array([[[[0.75, 0.5], [-1.0, 9.0]], [[0.125, 1.0], [0.5, 9.0]]]], f32)
    vol = cv.compute(a, mask, feat, other, 's', 1)['volume']
    assert vol.shape == (1, 9, 2, 2) and vol.dtype == f32
    want = np.zeros(9, f32)
    want[4] = (f32(0.5) * f32(0.75) + f32(-0.25) * f32(0.125)) / f32(2)                      # o = centre
    want[5] = (f32(0.5) * f32(0.5) + f32(-0.25) * f32(1.0)) / f32(2)                         # (0, +1)
    want[7] = (f32(0.5) * f32(-1.0) + f32(-0.25) * f32(0.5)) / f32(2)                        # (+1, 0)
    assert vol[0, :, 0, 0].tolist() == want.tolist() and not vol[0, 8, 0, 0]                  # (+1, +1) is masked
    assert not vol[0, :, 0, 1].any() and not vol[0, :, 1, :].any()                            # feat is 0 there
    nan_feat = feat.copy()
    nan_feat[0, 1, 1, 1] = np.nan                                                             # a NaN in feat: all D entries of its pixel
    vol = cv.compute(a, mask, nan_feat, other, 's', 1)['volume']
    assert np.isnan(vol[0, :, 1, 1]).all() and not np.isnan(vol[0, :, 0, :]).any() and not np.isnan(vol[0, :, 1, 0]).any()
    # a NaN and an inf in `other` at (3, 3) of a 4 x 4 frame under zero flow: the samples of (2, 2), (2, 3), (3, 2) and (3, 3) have it
    # among their taps (with weight 0 or 1); with those four masked it is selected out, not multiplied
    feat, other = (x[:1].copy() for x in cv.features(2, 2, 4, 4, 's'))
    other[0, :, 3, 3] = [np.nan, np.inf]
    mask = np.ones((1, 4, 4), bool)
    mask[0, 2:, 2:] = False
    res = cv.compute(np.zeros((1, 2, 4, 4), f32), mask, feat, other, 's', 1)
    assert np.array_equal(res['usable'], mask) and res['inside'].all()
    assert np.isfinite(res['volume']).all() and np.isfinite(res['warped']).all() and np.abs(res['volume']).max() > 0.1
    mask[0, 2, 2] = True
    assert np.isnan(cv.compute(np.zeros((1, 2, 4, 4), f32), mask, feat, other, 's', 1)['volume']).any()


# ---- host logic: the API with the native calls served by the oracle ------------------------------------------------------------------
def _flow(ref='s', n=2, h=20, w=28, mask=True):
    import oflibpytorch_amd as ofl
    a, m = cv.case(n, h, w, ref)
    return ofl.Flow(torch.from_numpy(a.copy()), ref, torch.from_numpy(m.copy()) if mask else None)


@pytest.mark.parametrize("ref", cv.REFS)
def test_volume_shape_dtype_and_values(cv_native, ref):
    n, c, h, w = 2, 3, 20, 28
    flow = _flow(ref)
    a, m = cv.case(n, h, w, ref)
    feat, other = cv.features(n, c, h, w, ref)
    vol = flow.cost_volume(torch.from_numpy(feat.copy()), torch.from_numpy(other.copy()))
    assert vol.dtype == torch.float32 and vol.shape == (n, 81, h, w) and not vol.requires_grad
    assert np.array_equal(vol.numpy(), cv.compute(a, m, feat, other, ref, 4)['volume'])       # the default: radius 4
    for radius in (1, 2, 3):
        vol = flow.cost_volume(feat.copy(), other.copy(), radius=radius)                      # arrays are taken
        assert np.array_equal(vol.numpy(), cv.compute(a, m, feat, other, ref, radius)['volume'])
    # consider_mask=False drops the mask; C-H-W features broadcast over the batch, one of them or both; non-contiguous ones are taken
    assert np.array_equal(flow.cost_volume(feat.copy(), other.copy(), 2, consider_mask=False).numpy(),
                          cv.compute(a, None, feat, other, ref, 2)['volume'])
    assert np.array_equal(flow.cost_volume(feat[0].copy(), other[0].copy(), 1).numpy(), cv.compute(a, m, feat[0], other[0], ref, 1)['volume'])
    assert np.array_equal(flow.cost_volume(feat.copy(), other[1].copy(), 1).numpy(), cv.compute(a, m, feat, other[1], ref, 1)['volume'])
    nhwc = [torch.from_numpy(x.copy()).contiguous(memory_format=torch.channels_last) for x in (feat, other)]
    assert np.array_equal(flow.cost_volume(*nhwc, radius=1).numpy(), cv.compute(a, m, feat, other, ref, 1)['volume'])
    one = torch.from_numpy(feat[:, :1].copy()), torch.from_numpy(other[:, :1].copy())
    assert np.array_equal(flow.cost_volume(*one, radius=3).numpy(), cv.compute(a, m, feat[:, :1], other[:, :1], ref, 3)['volume'])


def test_adapter_on_tensors_and_arrays(cv_native):
    import oflibpytorch_amd as ofl
    n, c, h, w = 2, 4, 20, 28
    a, m = cv.case(n, h, w, 't')
    feat, other = cv.features(n, c, h, w, 't')
    want = cv.compute(a, m, feat, other, 't', 2)['volume']
    got = ofl.flow_cost_volume(a.copy(), feat.copy(), other.copy(), 't', m.copy(), radius=2)
    assert isinstance(got, torch.Tensor) and got.shape == (n, 25, h, w) and np.array_equal(got.numpy(), want)
    one = ofl.flow_cost_volume(torch.from_numpy(a[1].copy()), torch.from_numpy(feat[1].copy()), torch.from_numpy(other[1].copy()), 't',
                               torch.from_numpy(m[1].copy()), 2)
    assert one.shape == (25, h, w) and np.array_equal(one.numpy(), want[1])
    got = ofl.flow_cost_volume(a.copy(), feat.copy(), other.copy(), 's')
    assert got.shape == (n, 81, h, w) and np.array_equal(got.numpy(), cv.compute(a, None, feat, other, 's', 4)['volume'])


@pytest.mark.parametrize("chw", [False, True], ids=["nchw", "chw"])
@pytest.mark.parametrize("ref", cv.REFS)
def test_inputs_that_require_a_gradient_go_through_cost_volume_fn(cv_native, monkeypatch, ref, chw):
    """The whole backward on the host: d feat and d W from the oracle, d other and d flow from its float64 backward of the warp in place
    of `_native.warp_bwd_grad`, against torch's float64 autograd of the definition; a C-H-W tensor gets its gradient summed over the
    batch, and what needs no gradient costs no call."""
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _autograd, _native
    calls = []

    def fake_warp_bwd_grad(flow, src, grad_out, *, flow_sign=1.0, g_scale=1.0, want_src=True, want_flow=True):
        calls.append((flow_sign, want_src, want_flow))
        assert src.dim() == 4 and g_scale == 1.0
        d_other, d_flow = cv.chain(flow.detach().numpy(), src.detach().numpy(), grad_out.numpy(), 's' if flow_sign < 0 else 't')
        return (torch.from_numpy(d_other).float() if want_src else None), (torch.from_numpy(d_flow).float() if want_flow else None)
    monkeypatch.setattr(_native, "warp_bwd_grad", fake_warp_bwd_grad)
    n, c, h, w, radius = 2, 3, 20, 28, 2
    a, m = cv.case(n, h, w, ref)
    feat, other = cv.features(n, c, h, w, ref)
    if chw:
        feat, other = feat[0], other[1]
    g = cv.upstream(n, 25, h, w)
    v = torch.from_numpy(a.copy()).requires_grad_(True)
    ft, ot = torch.from_numpy(feat.copy()).requires_grad_(True), torch.from_numpy(other.copy()).requires_grad_(True)
    vol = ofl.Flow(v, ref, torch.from_numpy(m.copy())).cost_volume(ft, ot, radius=radius)
    assert vol.requires_grad and type(vol.grad_fn).__name__ == "CostVolumeFnBackward"
    assert issubclass(_autograd.CostVolumeFn, torch.autograd.Function)
    res = cv.compute(a, m, feat, other, ref, radius)
    assert np.array_equal(vol.detach().numpy(), res['volume'])
    vol.backward(torch.from_numpy(g.copy()))
    assert calls == [(cv.sign_of(ref), True, True)]
    want = cv.torch_reference(a, res['usable'], feat, other, ref, radius, g)
    for name, got, ref64 in (("feat", ft.grad, want['d_feat']), ("other", ot.grad, want['d_other']), ("flow", v.grad, want['d_flow'])):
        scale = np.abs(ref64).max()
        assert got.dtype == torch.float32 and got.shape == ref64.shape and scale > 1e-2, name
        assert np.abs(got.numpy() - ref64).max() <= 2e-4 * scale, name
    # only feat wants a gradient: no backward of the warp; only the flow: no gradient of feat is formed
    ft2 = torch.from_numpy(feat.copy()).requires_grad_(True)
    ofl.Flow(torch.from_numpy(a.copy()), ref).cost_volume(ft2, torch.from_numpy(other.copy()), radius=1).sum().backward()
    assert len(calls) == 1 and ft2.grad is not None
    v2 = torch.from_numpy(a.copy()).requires_grad_(True)
    ofl.Flow(v2, ref).cost_volume(torch.from_numpy(feat.copy()), torch.from_numpy(other.copy()), radius=1).sum().backward()
    assert calls[1:] == [(cv.sign_of(ref), False, True)] and v2.grad is not None
    with torch.no_grad():
        assert not ofl.Flow(v, ref).cost_volume(ft, ot, radius=1).requires_grad and len(calls) == 2


# ---- the checks of the API, none of which needs a device ------------------------------------------------------------------------------
def test_api_checks_and_their_messages(oracle_native, monkeypatch):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _cost_volume

    def never(*args, **kw):
        raise AssertionError("the checks come before the kernel")
    monkeypatch.setattr(_cost_volume, "flow_cost_volume", never)
    monkeypatch.setattr(_cost_volume, "cost_volume", never)
    flow = _flow(n=2, h=6, w=7)
    pre = r"Error computing cost volume: "
    good = torch.zeros(2, 5, 6, 7)
    call = flow.cost_volume
    for name, both in (("Feat", lambda bad: (bad, good)), ("Other", lambda bad: (good, bad))):
        for bad in ("feat", [1.0], 3, None):
            with pytest.raises(TypeError, match=pre + name + " needs to be a torch tensor or a numpy array"):
                call(*both(bad))
        for bad in (good.double(), good.half(), good.bfloat16(), good.to(torch.uint8), good.to(torch.int32), np.zeros((2, 5, 6, 7)),
                    np.zeros((2, 5, 6, 7), np.uint8)):
            with pytest.raises(TypeError, match=pre + name + " needs to be of dtype float32"):
                call(*both(bad))
        for bad in (torch.zeros(6, 7), torch.zeros(1, 2, 5, 6, 7)):
            with pytest.raises(ValueError, match=pre + name + " needs to have 3 or 4 dimensions"):
                call(*both(bad))
        for bad in (torch.zeros(2, 0, 6, 7), torch.zeros(0, 6, 7)):
            with pytest.raises(ValueError, match=pre + name + " needs to have at least 1 channel"):
                call(*both(bad))
        for bad in (torch.zeros(2, 5, 7, 6), torch.zeros(5, 6, 8)):
            with pytest.raises(ValueError, match=pre + name + " needs to have the H-W shape of the flow"):
                call(*both(bad))
        for bad in (torch.zeros(1, 5, 6, 7), torch.zeros(3, 5, 6, 7)):
            with pytest.raises(ValueError, match=pre + name + " needs to have the batch size of the flow"):
                call(*both(bad))
    with pytest.raises(ValueError, match=pre + "Feat and other need to have the same number of channels"):
        call(good, torch.zeros(2, 4, 6, 7))
    for bad in (True, "3", 3.0, [3], torch.tensor(3)):
        with pytest.raises(TypeError, match=pre + "Radius needs to be an integer"):
            call(good, good, radius=bad)
    for bad in (0, -1, 5, 9, 81):
        with pytest.raises(ValueError, match=pre + "Radius needs to be 1, 2, 3 or 4"):
            call(good, good, radius=bad)
    for bad in (1, 0, "True", 1.0):
        with pytest.raises(TypeError, match=pre + "Consider_mask needs to be boolean"):
            call(good, good, consider_mask=bad)
    # the order: types and dtypes, shapes, the frame's size, radius, consider_mask
    with pytest.raises(TypeError, match="dtype"):
        call(good, torch.zeros(2, 9, 6, 7, dtype=torch.uint8), radius="x")
    with pytest.raises(ValueError, match="channels"):
        call(good, torch.zeros(2, 9, 6, 7), radius="x")
    with pytest.raises(TypeError, match="Radius"):
        call(good, good, radius="x", consider_mask=1)
    thin = ofl.Flow(torch.zeros(2, 2, 1, 7), 't')
    with pytest.raises(ValueError, match=pre + "Flow field needs to be at least 2 pixels high and wide"):
        thin.cost_volume(torch.zeros(2, 5, 1, 7), torch.zeros(2, 5, 1, 7), radius="x")
    with pytest.raises(ValueError, match=pre):
        ofl.flow_cost_volume(flow.vecs, good, good, 't', radius=7)
    with pytest.raises(TypeError, match=pre):
        ofl.flow_cost_volume(flow.vecs, good, good.double(), 's')


def test_the_gradient_binding_wants_an_output():
    from oflibpytorch_amd import _cost_volume
    v, good = torch.zeros(2, 2, 6, 7), torch.zeros(2, 5, 6, 7)
    with pytest.raises(ValueError, match="at least one output"):
        _cost_volume.flow_cost_volume_grad(v, None, good, good, -1.0, 1, torch.zeros(2, 9, 6, 7), want_feat=False, want_warped=False)


def test_the_method_and_adapter_are_exported():
    import oflibpytorch_amd as ofl
    assert callable(ofl.Flow.cost_volume) and callable(ofl.flow_cost_volume)
    assert "Differentiable with respect to `feat`, `other` and the flow" in " ".join(ofl.Flow.cost_volume.__doc__.split())


# ---- the C ABI: declared, exported, and every rejected argument is rejected before any launch --------------------------------------
def test_c_abi_declarations_and_argument_checks_need_no_gpu():
    from oflibpytorch_amd import _cost_volume, _native
    names = {"ofl_flow_cost_volume_f32", "ofl_flow_cost_volume_grad_f32", "ofl_flow_cost_volume_chain_f32", "ofl_flow_cost_volume_gate_f32"}
    assert names <= set(_native.exported_symbols())
    header = open(_native._build.HEADERS[0]).read()
    for name in names:
        assert (" %s(" % name) in header
    assert (_cost_volume.RADIUS, _cost_volume.MAX_RADIUS) == (cv.RADIUS, max(cv.RADII)) == (4, 4)
    assert any(src.endswith("ofl_cost_volume.hip") for src in _native._build.SOURCES)
    lib = _cost_volume._library()
    assert lib.ofl_version() == _native.ABI_VERSION                      # names were added, no signature changed
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(4096)      # never dereferenced: every call below is rejected first

    def fwd(flow=one, flow_bs=0, half=0, mask=null, mask_bs=0, feat=one, feat_bs=0, other=one, other_bs=0, chan=8, sign=-1.0, radius=4,
            vol=one, n=1, h=4, w=4):
        return lib.ofl_flow_cost_volume_f32(flow, flow_bs, half, mask, mask_bs, feat, feat_bs, other, other_bs, chan, sign, radius, vol,
                                            n, h, w, null)

    def bwd(flow=one, flow_bs=0, half=0, mask=null, mask_bs=0, feat=one, feat_bs=0, other=one, other_bs=0, chan=8, sign=-1.0, radius=4,
            g=one, d_feat=one, d_w=one, n=1, h=4, w=4):
        return lib.ofl_flow_cost_volume_grad_f32(flow, flow_bs, half, mask, mask_bs, feat, feat_bs, other, other_bs, chan, sign, radius,
                                                 g, d_feat, d_w, n, h, w, null)
    odd = ctypes.c_void_p(4098)
    nan = float('nan')
    shared = (dict(n=0), dict(n=65536), dict(n=-3), dict(h=1), dict(w=1), dict(h=0), dict(h=65536, w=32768), dict(h=46341, w=46341),
              dict(sign=0.0), dict(sign=2.0), dict(sign=-0.5), dict(sign=nan),
              dict(chan=0), dict(chan=-1), dict(radius=0), dict(radius=5), dict(radius=-1), dict(radius=9),
              dict(flow=null), dict(feat=null), dict(other=null),
              dict(flow_bs=-1), dict(mask_bs=-32), dict(feat_bs=-1), dict(other_bs=-8), dict(half=2), dict(half=-1),
              dict(flow=odd), dict(flow=ctypes.c_void_p(4097), half=1), dict(feat=odd), dict(other=odd))
    for kw in shared + (dict(vol=null), dict(vol=odd)):
        assert fwd(**kw) == -3, kw
    for kw in shared + (dict(g=null), dict(g=odd), dict(d_feat=null, d_w=null), dict(d_feat=odd), dict(d_w=odd)):
        assert bwd(**kw) == -3, kw

    def chain(flow=one, flow_bs=0, half=0, sign=-1.0, out=one, n=1, h=4, w=4):
        return lib.ofl_flow_cost_volume_chain_f32(flow, flow_bs, half, sign, out, n, h, w, null)

    def gate(flow=one, flow_bs=0, half=0, mask=null, mask_bs=0, sign=-1.0, out=one, n=1, h=4, w=4):
        return lib.ofl_flow_cost_volume_gate_f32(flow, flow_bs, half, mask, mask_bs, sign, out, n, h, w, null)
    flow_only = (dict(n=0), dict(n=65536), dict(h=1), dict(w=1), dict(h=46341, w=46341), dict(sign=0.0), dict(sign=nan), dict(flow=null),
                 dict(flow_bs=-1), dict(half=2), dict(flow=odd), dict(out=null), dict(out=odd))
    for kw in flow_only:
        assert chain(**kw) == -3, kw
    for kw in flow_only + (dict(mask_bs=-32),):
        assert gate(**kw) == -3, kw
