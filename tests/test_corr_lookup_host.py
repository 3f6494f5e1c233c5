"""CPU tier of Flow.corr_lookup: the oracle (tests/corr_lookup_oracle.py) against the expression people mean (RAFT's
all-pairs volume, pooled, sampled by grid_sample, in float64), its float32 order against its float64 evaluation within the derived
bound, its gradients against torch's float64 autograd, a hand-computed pixel, RAFT's channel order, the coverage condition of the GPU
tier's inputs, the host logic of the API with the native calls served by the oracle, every argument check that needs no device, and the
C ABI's declarations and argument checks.  No device."""
import ctypes

import numpy as np
import pytest
import torch

import corr_lookup_oracle as cl

GPU_FRAMES = cl.frames()
U = 2.0 ** -24                                           # the unit roundoff of float32


@pytest.fixture
def cl_native(oracle_native, monkeypatch):
    from oflibpytorch_amd import _corr_lookup
    monkeypatch.setattr(_corr_lookup, "flow_corr_lookup", cl.fake_flow_corr_lookup)
    monkeypatch.setattr(_corr_lookup, "flow_corr_lookup_grad", cl.fake_flow_corr_lookup_grad)
    return _corr_lookup


def _exact_case(n, h, w, seed, reach=63):
    """Vectors on a grid of 2^-6 with |a| < 64 (every position step is exact in float32) and a mask"""
    rng = np.random.RandomState(seed)
    a = (rng.randint(-reach * 64, reach * 64 + 1, (n, 2, h, w)) / 64.0).astype(np.float32)
    a[:, :, :h // 2] /= 8                                                                     # half of them stay near the frame
    return a, rng.uniform(size=(n, h, w)) >= 0.2


# ---- the oracle computes the expression people mean ----------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", cl.RADII)
@pytest.mark.parametrize("ref", cl.REFS)
def test_float64_evaluation_is_the_all_pairs_lookup(ref, radius):
    """11 x 13 (odd sizes: the pooling floors), C = 5, three levels pooled in float64: the oracle's float64 evaluation against the
    all-pairs / avg_pool2d / grid_sample expression within 1e-12 of the volume's scale (under 1000 float64 roundings of 1.1e-16)."""
    n, c, h, w, levels = 2, 5, 11, 13, 3
    a, mask = _exact_case(n, h, w, 17 + radius)
    feat, other = cl.features(n, c, h, w, ref), cl.features(n, c, h, w, ref, salt=1)
    got = cl.compute(a, mask, feat, cl.pyramid(other, levels, float64=True), ref, radius, float64=True)
    want = cl.torch_reference(a, mask, feat, other, ref, radius, levels=levels)['lookup']
    assert got['lookup'].dtype == np.float64 and got['lookup'].shape == want.shape == (n, levels * (2 * radius + 1) ** 2, h, w)
    scale = np.abs(want).max()
    err = np.abs(got['lookup'] - want).max()
    print("'%s' radius %d: largest |oracle float64 - all-pairs lookup| = %.3e of a scale %.3e" % (ref, radius, err, scale))
    assert scale > 0.1 and err <= 1e-12 * scale
    assert got['any_inside'].mean() > 0.2 and (~got['any_inside']).mean() > 0.05 and 0.5 < got['usable'].mean() < 0.95


def test_float32_definition_against_its_float64_evaluation():
    """Per entry: C products and C sums from +0 (the first is exact), then one product, three fused multiply-adds, one square root and
    one division on float32 weights that both evaluations share: at most C + 6 roundings, each at most 2^-24 of the sum of the terms'
    absolute values; (C + 8) 2^-24 covers the second-order terms."""
    worst = 0.0
    for (n, h, w), c in zip(GPU_FRAMES, (3, 16, 1, 35, 17, 4, 15)):
        for ref in cl.REFS:
            a, m = cl.case(n, h, w, ref)
            feat, lv = cl.explicit_levels(n, c, h, w, ref)
            for radius in (1, 4):
                r32 = cl.compute(a, m, feat, lv, ref, radius)['lookup']
                r64 = cl.compute(a, m, feat, lv, ref, radius, float64=True)['lookup']
                mag = cl.compute(a, m, np.abs(feat), [np.abs(x) for x in lv], ref, radius, float64=True)['lookup']
                assert r32.dtype == np.float32 and r32.shape == (n, 4 * (2 * radius + 1) ** 2, h, w)
                bound = (c + 8) * U * mag
                err = np.abs(r32.astype(np.float64) - r64)
                assert np.all(err <= bound), (n, h, w, ref, radius, float((err - bound).max()))
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print("largest |float32 lookup - float64 evaluation| is %.3f of the bound" % worst)
    assert worst > 0


# ---- the oracle's gradients are the derivative ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 4])
@pytest.mark.parametrize("ref", cl.REFS)
def test_oracle_gradients_are_the_float64_derivative(ref, radius):
    """9 x 13, exact positions.  The float64 evaluation of the oracle's gradients is torch's float64 autograd of the all-pairs expression
    within 1e-12 of its scale.  The float32 gradients are within (m + 10) 2^-24 of the sum of the terms' absolute values of that
    evaluation, m the number of products a sum can hold: one square root, one division, four products and four sums in Gn, then one
    product and one sum per term -- m = L (2 r + 2)^2 for d feat and (2 r + 2)^2 H W for d other."""
    n, c, h, w = 2, 3, 9, 13
    a, mask = _exact_case(n, h, w, 41 + radius, reach=20)
    feat = cl.features(n, c, h, w, ref)
    lv = [cl.features(n, c, hl, wl, ref, salt=l + 1) for l, (hl, wl) in enumerate([(h, w), (4, 6), (1, 1)])]
    k, d = (2 * radius + 2) ** 2, (2 * radius + 1) ** 2
    g = cl.upstream(n, len(lv) * d, h, w)
    want = cl.torch_reference(a, mask, feat, lv, ref, radius, g=g)
    f64, l64 = cl.grads(a, mask, feat, lv, ref, radius, g, float64=True)
    f32, l32 = cl.grads(a, mask, feat, lv, ref, radius, g)
    big_f, big_l = cl.grads(a, mask, np.abs(feat), [np.abs(x) for x in lv], ref, radius, np.abs(g), float64=True)
    assert f32.dtype == np.float32 and all(x.dtype == np.float32 for x in l32)
    for name, got64, got32, ref64, big, m in [("d feat", f64, f32, want['d_feat'], big_f, len(lv) * k)] + [
            ("d other %d" % l, l64[l], l32[l], want['d_other'][l], big_l[l], k * h * w) for l in range(len(lv))]:
        scale = np.abs(ref64).max()
        print("'%s' radius %d %s: float64 error %.3e, float32 error %.3e of a scale %.3e" % (
            ref, radius, name, np.abs(got64 - ref64).max(), np.abs(got32 - got64).max(), scale))
        assert scale > 1e-2 and np.abs(got64 - ref64).max() <= 1e-12 * scale, name
        assert np.all(np.abs(got32.astype(np.float64) - got64) <= (m + 10) * U * big), name
    unusable = ~np.broadcast_to(cl.window(a, mask, ref, 0)['usable'][:, None], f32.shape)
    assert unusable.mean() > 0.1 and not f32[unusable].view(np.uint32).any() and not want['d_feat'][unusable].any()


# ---- the coverage condition of the GPU tier's inputs ----------------------------------------------------------------------------------
def test_every_gpu_frame_of_9_by_9_and_larger_shows_every_category():
    """No GPU test can pass on an empty set.  Per frame of at least 9 x 9 and for both refs, on level 0 with radius 1 (a 4 x 4 window,
    which fits every such frame): a window fully inside, one across each of the four edges, one fully outside, a masked pixel, an
    integer position and a negative position."""
    checked = 0
    for n, h, w in GPU_FRAMES:
        if h < 9 or w < 9:
            continue
        for ref in cl.REFS:
            a, m = cl.case(n, h, w, ref)
            cats = cl.categories(a, m, ref, 1, h, w)
            counts = {k: int(v.sum()) for k, v in cats.items()}
            print("%d x %d x %d '%s': %s" % (n, h, w, ref, counts))
            assert set(counts) == {'inside', 'outside', 'north', 'south', 'west', 'east', 'masked', 'integer', 'negative'}
            assert min(counts.values()) >= 1, (n, h, w, ref, counts)
            checked += 1
    assert checked >= 4
    for n, h, w in GPU_FRAMES:                                                                # the vectors survive fp16 storage
        a = cl.case(n, h, w, 's')[0]
        assert np.array_equal(a.astype(np.float16).astype(np.float32), a)


def test_the_smooth_and_the_one_cell_flows_are_what_they_say():
    a, _ = cl.one_cell_case(1, 16, 32, 's')
    win = cl.window(a, None, 's', 0)
    assert np.unique(win['x_w']).tolist() == [16.0] and np.unique(win['y_n']).tolist() == [8.0] and win['usable'].all()
    assert len(np.unique(win['nw'])) > 4
    a, _ = cl.one_cell_case(1, 16, 32, 't')
    assert np.array_equal(cl.window(a, None, 't', 0)['x_w'], win['x_w'])
    a, _ = cl.smooth_case(1, 17, 33, 's')
    win = cl.window(a, None, 's', 0)
    assert np.abs(np.diff(win['x_w'], axis=2)).max() <= 2 and np.abs(np.diff(win['y_n'], axis=1)).max() <= 2


# ---- known answers ------------------------------------------------------------------------------------------------------------------
def test_hand_computed_pixel():
    """A 2 x 3 frame, two channels, radius 1, one level, the vector (0.5, 0.25) at pixel (0, 0) of an 's' flow: position (0.5, 0.25),
    x_w = y_n = 0, ww = 0.5, nn = 0.25.  Entry (dx, dy) = (0, 0) is the bilinear sample of feat . other over the nodes (0..1, 0..1),
    entry (-1, 0) reads column -1 as zero, and all is divided by sqrt(2)."""
    f32 = np.float32
    a = np.zeros((1, 2, 2, 3), f32)
    a[0, :, 0, 0] = [0.5, 0.25]
    feat = np.zeros((1, 2, 2, 3), f32)
    feat[0, :, 0, 0] = [0.5, -0.25]
    other = np.array([[[[0.75, 0.5, 2.0], [-1.0, 9.0, 3.0]], [[0.125, 1.0, 4.0], [0.5, 8.0, 5.0]]]], f32)
    out = cl.compute(a, None, feat, [other], 's', 1)['lookup']
    assert out.shape == (1, 9, 2, 3) and out.dtype == f32
    k = lambda y, x: f32(0.5) * other[0, 0, y, x] + f32(-0.25) * other[0, 1, y, x]
    nw, ne, sw, se = f32(0.75 * 0.5), f32(0.75 * 0.5), f32(0.25 * 0.5), f32(0.25 * 0.5)
    root = np.sqrt(f32(2))
    centre = (k(0, 0) * nw + k(0, 1) * ne + k(1, 0) * sw + k(1, 1) * se) / root              # (every step exact here but the division)
    west = (k(0, 0) * ne + k(1, 0) * se) / root
    east = (k(0, 1) * nw + k(0, 2) * ne + k(1, 1) * sw + k(1, 2) * se) / root
    south = (k(1, 0) * nw + k(1, 1) * ne) / root
    assert out[0, 4, 0, 0] == centre and out[0, 1, 0, 0] == west and out[0, 7, 0, 0] == east and out[0, 5, 0, 0] == south
    assert out[0, 0, 0, 0] == (k(0, 0) * se) / root != 0                                      # (-1, -1): one node inside, (0, 0), weight se
    assert not out[0, :, 1, :].any() and not out[0, :, 0, 1:].any()                           # feat is 0 there
    # a masked pixel: +0 whatever the features hold; a NaN vector the same
    nan_feat = np.full_like(feat, np.nan)
    assert not cl.compute(a, np.zeros((1, 2, 3), bool), nan_feat, [other], 's', 1)['lookup'].view(np.uint32).any()
    bad = a.copy()
    bad[0, 1] = np.nan
    assert not cl.compute(bad, None, nan_feat, [other], 's', 1)['lookup'].view(np.uint32).any()
    # a 't' flow looks at p - a(p)
    assert np.array_equal(cl.compute(-a, None, feat, [other], 't', 1)['lookup'], out)


@pytest.mark.parametrize("radius", cl.RADII)
def test_the_x_offset_is_the_outer_index(radius):
    """An impulse in `other` at (y0, x0), zero flow, feat = 1: pixel p sees it at the offset (dx, dy) = (x0 - px, y0 - py) alone, which
    is entry (dx + r)(2 r + 1) + dy + r -- RAFT's order, not the cost volume's."""
    h, w, y0, x0 = 11, 12, 6, 4
    other = np.zeros((1, 1, h, w), np.float32)
    other[0, 0, y0, x0] = 1.0
    out = cl.compute(np.zeros((1, 2, h, w), np.float32), None, np.ones((1, 1, h, w), np.float32), [other], 's', radius)['lookup']
    win = 2 * radius + 1
    for py in range(h):
        for px in range(w):
            dx, dy = x0 - px, y0 - py
            want = np.zeros(win * win, np.float32)
            if abs(dx) <= radius and abs(dy) <= radius:
                want[(dx + radius) * win + dy + radius] = 1.0
            assert np.array_equal(out[0, :, py, px], want), (py, px)
    asym = out[0, (1 + radius) * win + radius]                                                # (dx, dy) = (1, 0): the pixel west of the impulse
    assert asym[y0, x0 - 1] == 1.0 and asym.sum() == 1.0


# ---- host logic: the API with the native calls served by the oracle ------------------------------------------------------------------
def _flow(ref='s', n=2, h=20, w=28, mask=True):
    import oflibpytorch_amd as ofl
    a, m = cl.case(n, h, w, ref)
    return ofl.Flow(torch.from_numpy(a.copy()), ref, torch.from_numpy(m.copy()) if mask else None)


@pytest.mark.parametrize("ref", cl.REFS)
def test_lookup_shape_dtype_and_values(cl_native, ref):
    import oflibpytorch_amd as ofl
    n, c, h, w = 2, 3, 20, 28
    flow = _flow(ref)
    a, m = cl.case(n, h, w, ref)
    feat, other = cl.features(n, c, h, w, ref), cl.features(n, c, h, w, ref, salt=1)
    out = flow.corr_lookup(torch.from_numpy(feat.copy()), torch.from_numpy(other.copy()))
    assert out.dtype == torch.float32 and out.shape == (n, 4 * 81, h, w) and not out.requires_grad       # the defaults: radius 4, 4 levels
    assert np.array_equal(out.numpy(), cl.compute(a, m, feat, cl.pyramid(other, 4), ref, 4)['lookup'])
    out = flow.corr_lookup(feat.copy(), other.copy(), radius=2, levels=2, consider_mask=False)            # arrays are taken
    assert np.array_equal(out.numpy(), cl.compute(a, None, feat, cl.pyramid(other, 2), ref, 2)['lookup'])
    # a sequence of levels of any sizes; `levels` is ignored; C-H-W tensors broadcast over the batch
    _, lv = cl.explicit_levels(n, c, h, w, ref)
    out = flow.corr_lookup(feat[0].copy(), [lv[0].copy(), lv[1][1].copy(), lv[2].copy(), lv[3].copy()], radius=1, levels=1)
    assert out.shape == (n, 4 * 9, h, w)
    assert np.array_equal(out.numpy(), cl.compute(a, m, feat[0], [lv[0], lv[1][1], lv[2], lv[3]], ref, 1)['lookup'])
    pyr = ofl.corr_pyramid(torch.from_numpy(other.copy()), 3)
    assert [tuple(x.shape) for x in pyr] == [(n, c, 20, 28), (n, c, 10, 14), (n, c, 5, 7)]
    assert np.array_equal(flow.corr_lookup(feat.copy(), pyr, radius=3).numpy(), flow.corr_lookup(feat.copy(), other.copy(), 3, 3).numpy())
    got = ofl.flow_corr_lookup(a[1].copy(), feat[1].copy(), other[1].copy(), ref, m[1].copy(), radius=1, levels=2)
    assert got.shape == (2 * 9, h, w)
    assert np.array_equal(got.numpy(), cl.compute(a[1:], m[1:], feat[1:], cl.pyramid(other[1:], 2), ref, 1)['lookup'][0])


@pytest.mark.parametrize("chw", [False, True], ids=["nchw", "chw"])
@pytest.mark.parametrize("ref", cl.REFS)
def test_inputs_that_require_a_gradient_go_through_corr_lookup_fn(cl_native, ref, chw):
    """The whole backward on the host: the oracle's gradients behind CorrLookupFn, torch's autograd through the pooling, against the
    float64 autograd of the all-pairs expression within 2e-4 of each gradient's scale; a C-H-W tensor gets its gradient summed over the
    batch; the vectors get none."""
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _autograd
    n, c, h, w, radius, levels = 2, 3, 12, 14, 2, 3
    a, m = cl.case(n, h, w, ref)
    feat, other = cl.features(n, c, h, w, ref), cl.features(n, c, h, w, ref, salt=1)
    if chw:
        feat, other = feat[0], other[1]
    g = cl.upstream(n, levels * 25, h, w)
    v = torch.from_numpy(a.copy()).requires_grad_(True)
    ft, ot = torch.from_numpy(feat.copy()).requires_grad_(True), torch.from_numpy(other.copy()).requires_grad_(True)
    out = ofl.Flow(v, ref, torch.from_numpy(m.copy())).corr_lookup(ft, ot, radius=radius, levels=levels)
    assert out.requires_grad and type(out.grad_fn).__name__ == "CorrLookupFnBackward"
    assert issubclass(_autograd.CorrLookupFn, torch.autograd.Function)
    out.backward(torch.from_numpy(g.copy()))
    assert v.grad is None
    want = cl.torch_reference(a, m, feat, other, ref, radius, levels=levels, g=g)
    for name, got, ref64 in (("feat", ft.grad, want['d_feat']), ("other", ot.grad, want['d_other'])):
        scale = np.abs(ref64).max()
        assert got.dtype == torch.float32 and got.shape == ref64.shape and scale > 1e-2, name
        assert np.abs(got.numpy() - ref64).max() <= 2e-4 * scale, name
    # only one level wants a gradient: the others get None, and so does feat
    _, lv = cl.explicit_levels(n, c, h, w, ref)
    lv = [torch.from_numpy(x.copy()) for x in lv]
    lv[2].requires_grad_(True)
    ofl.Flow(torch.from_numpy(a.copy()), ref).corr_lookup(torch.from_numpy(cl.features(n, c, h, w, ref).copy()), lv, radius=1).sum().backward()
    assert lv[2].grad is not None and lv[2].grad.shape == lv[2].shape and lv[0].grad is None
    with torch.no_grad():
        assert not ofl.Flow(v, ref).corr_lookup(ft, ot, radius=1, levels=1).requires_grad


# ---- the checks of the API, none of which needs a device ------------------------------------------------------------------------------
def test_api_checks_and_their_messages(oracle_native, monkeypatch):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _corr_lookup

    def never(*args, **kw):
        raise AssertionError("the checks come before the kernel")
    monkeypatch.setattr(_corr_lookup, "flow_corr_lookup", never)
    monkeypatch.setattr(_corr_lookup, "corr_lookup", never)
    flow = _flow(n=2, h=6, w=7)
    pre = r"Error computing correlation lookup: "
    good = torch.zeros(2, 5, 6, 7)
    call = flow.corr_lookup
    for name, both in (("Feat", lambda bad: (bad, good)), ("Other", lambda bad: (good, bad))):
        for bad in ("feat", 3, None):
            with pytest.raises(TypeError, match=pre + name + " needs to be a torch tensor or a numpy array"):
                call(*both(bad))
        for bad in (good.double(), good.half(), good.bfloat16(), good.to(torch.uint8), np.zeros((2, 5, 6, 7))):
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
    with pytest.raises(ValueError, match=pre + "Feat and other need to have the same number of channels"):
        call(good, [good, torch.zeros(2, 4, 3, 3)])
    for bad in ([], [good] * 7):
        with pytest.raises(ValueError, match=pre + "Other needs to hold 1 to 6 levels"):
            call(good, bad)
    with pytest.raises(ValueError, match=pre + "Other level 1 is empty"):
        call(good, [good, torch.zeros(2, 5, 0, 3)])
    with pytest.raises(TypeError, match=pre + "Other level 1 needs to be of dtype float32"):
        call(good, [good, good.double()])
    with pytest.raises(ValueError, match=pre + "Other level 0 needs to have the batch size of the flow"):
        call(good, [torch.zeros(3, 5, 6, 7)])
    for bad in (True, "3", 3.0, [3]):
        with pytest.raises(TypeError, match=pre + "Radius needs to be an integer"):
            call(good, good, radius=bad)
    for bad in (0, -1, 5, 9):
        with pytest.raises(ValueError, match=pre + "Radius needs to be 1, 2, 3 or 4"):
            call(good, good, radius=bad)
    for bad in (True, "3", 3.0):
        with pytest.raises(TypeError, match=pre + "Levels needs to be an integer"):
            call(good, good, levels=bad)
    for bad in (0, -1, 7):
        with pytest.raises(ValueError, match=pre + "Levels needs to be 1 to 6"):
            call(good, good, levels=bad)
    with pytest.raises(ValueError, match=pre + "Other level 3 is empty"):                     # 6 x 7 -> 3 x 3 -> 1 x 1 -> nothing
        call(good, good, levels=4)
    for bad in (1, 0, "True"):
        with pytest.raises(TypeError, match=pre + "Consider_mask needs to be boolean"):
            call(good, good, levels=2, consider_mask=bad)
    with pytest.raises(ValueError, match=pre):
        ofl.flow_corr_lookup(flow.vecs, good, good, 't', radius=7)
    with pytest.raises(TypeError, match=pre):
        ofl.flow_corr_lookup(flow.vecs, good, good.double(), 's')
    # the bindings and the pyramid check for themselves
    for bad, exc in ((True, TypeError), (2.0, TypeError), (0, ValueError), (7, ValueError)):
        with pytest.raises(exc, match="levels needs to be"):
            ofl.corr_pyramid(good, bad)
    with pytest.raises(ValueError, match="a level of the pyramid is empty"):
        ofl.corr_pyramid(good, 4)
    with pytest.raises(TypeError, match="need to be float32"):
        _corr_lookup.check_levels(good, [good.double()])
    with pytest.raises(ValueError, match="the same number of channels"):
        _corr_lookup.check_levels(good, [torch.zeros(2, 4, 6, 7)])
    with pytest.raises(ValueError, match="a level of the pyramid is empty"):
        _corr_lookup.check_levels(good, [torch.zeros(2, 5, 6, 0)])
    with pytest.raises(ValueError, match="1 to 6 levels"):
        _corr_lookup.check_levels(good, [])
    with pytest.raises(ValueError, match="at least one output"):
        _corr_lookup.flow_corr_lookup_grad(flow.vecs, None, good, [good], -1.0, 1, torch.zeros(2, 9, 6, 7), want_feat=False, want_levels=[False])


def test_the_method_the_adapter_and_the_pyramid_are_exported():
    import oflibpytorch_amd as ofl
    assert callable(ofl.Flow.corr_lookup) and callable(ofl.flow_corr_lookup) and callable(ofl.corr_pyramid)
    doc = " ".join(ofl.Flow.corr_lookup.__doc__.split())
    assert "NOT differentiable with respect to the flow vectors" in doc and "the x offset is the outer index" in doc
    assert "corr_lookup" in ofl.__doc__


# ---- the C ABI: declared, exported, and every rejected argument is rejected before any launch --------------------------------------
def test_c_abi_declarations_and_argument_checks_need_no_gpu():
    from oflibpytorch_amd import _corr_lookup, _native
    names = {"ofl_flow_corr_lookup_cells", "ofl_flow_corr_lookup_f32", "ofl_flow_corr_lookup_nodes_f32", "ofl_flow_corr_lookup_grad_feat_f32",
             "ofl_flow_corr_lookup_grad_other_f32"}
    assert names <= set(_native.exported_symbols())
    header = open(_native._build.HEADERS[0]).read()
    for name in names:
        assert (" %s(" % name) in header
    assert (_corr_lookup.RADIUS, _corr_lookup.MAX_RADIUS, _corr_lookup.LEVELS, _corr_lookup.MAX_LEVELS) == \
        (cl.RADIUS, max(cl.RADII), cl.LEVELS, cl.MAX_LEVELS) == (4, 4, 4, 6)
    assert any(src.endswith("ofl_corr_lookup.hip") for src in _native._build.SOURCES)
    lib = _corr_lookup._library()
    assert lib.ofl_version() == _native.ABI_VERSION == 36                # names were added, no signature changed
    assert lib.ofl_flow_corr_lookup_cells(20, 28, 4) == 29 * 37 + 1 and lib.ofl_flow_corr_lookup_cells(1, 1, 1) == 4 * 4 + 1
    for bad in ((0, 5, 1), (5, 0, 1), (5, 5, 0), (5, 5, 5), ((1 << 24) + 1, 1, 1), (1 << 16, 1 << 15, 1)):
        assert lib.ofl_flow_corr_lookup_cells(*bad) == -3, bad
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(4096)      # never dereferenced: every call below is rejected first
    odd, odd8 = ctypes.c_void_p(4098), ctypes.c_void_p(4100)
    nan = float('nan')

    def fwd(flow=one, flow_bs=0, half=0, mask=null, mask_bs=0, feat=one, feat_bs=0, other=one, other_bs=0, chan=8, sign=-1.0, radius=4,
            level=0, hl=4, wl=4, out=one, out_bs=81 * 16, n=1, h=4, w=4):
        return lib.ofl_flow_corr_lookup_f32(flow, flow_bs, half, mask, mask_bs, feat, feat_bs, other, other_bs, chan, sign, radius, level,
                                            hl, wl, out, out_bs, n, h, w, null)

    def nodes(flow=one, flow_bs=0, half=0, mask=null, mask_bs=0, chan=8, sign=-1.0, radius=4, level=0, hl=4, wl=4, g=one, g_bs=81 * 16,
              gn=one, keys=one, n=1, h=4, w=4):
        return lib.ofl_flow_corr_lookup_nodes_f32(flow, flow_bs, half, mask, mask_bs, chan, sign, radius, level, hl, wl, g, g_bs, gn, keys,
                                                  n, h, w, null)

    def d_feat(flow=one, flow_bs=0, half=0, mask=null, mask_bs=0, other=one, other_bs=0, chan=8, sign=-1.0, radius=4, level=0, hl=4,
               wl=4, gn=one, grad=one, acc=0, n=1, h=4, w=4):
        return lib.ofl_flow_corr_lookup_grad_feat_f32(flow, flow_bs, half, mask, mask_bs, other, other_bs, chan, sign, radius, level, hl,
                                                      wl, gn, grad, acc, n, h, w, null)

    def d_other(feat=one, feat_bs=0, chan=8, radius=4, hl=4, wl=4, gn=one, order=one, starts=one, grad=one, n=1, h=4, w=4):
        return lib.ofl_flow_corr_lookup_grad_other_f32(feat, feat_bs, chan, radius, hl, wl, gn, order, starts, grad, n, h, w, null)
    frame = (dict(n=0), dict(n=65536), dict(n=-3), dict(h=0), dict(w=0), dict(h=65536, w=32768), dict(h=46341, w=46341),
             dict(chan=0), dict(chan=-1), dict(radius=0), dict(radius=5), dict(radius=-1),
             dict(hl=0), dict(wl=0), dict(hl=(1 << 24) + 1), dict(hl=65536, wl=32768))
    with_flow = frame + (dict(sign=0.0), dict(sign=2.0), dict(sign=nan), dict(level=-1), dict(level=6), dict(flow=null), dict(flow_bs=-1),
                         dict(mask_bs=-32), dict(half=2), dict(half=-1), dict(flow=odd), dict(flow=ctypes.c_void_p(4097), half=1))
    for kw in with_flow + (dict(feat=null), dict(other=null), dict(out=null), dict(feat_bs=-1), dict(other_bs=-8), dict(feat=odd),
                           dict(other=odd), dict(out=odd), dict(out_bs=81 * 16 - 1), dict(out_bs=-1)):
        assert fwd(**kw) == -3, kw
    for kw in with_flow + (dict(g=null), dict(gn=null), dict(g=odd), dict(gn=odd), dict(keys=odd8), dict(g_bs=81 * 16 - 1)):
        assert nodes(**kw) == -3, kw
    for kw in with_flow + (dict(other=null), dict(gn=null), dict(grad=null), dict(other_bs=-1), dict(acc=2), dict(acc=-1), dict(other=odd),
                           dict(gn=odd), dict(grad=odd)):
        assert d_feat(**kw) == -3, kw
    for kw in frame + (dict(feat=null), dict(gn=null), dict(order=null), dict(starts=null), dict(grad=null), dict(feat_bs=-1),
                       dict(feat=odd), dict(gn=odd), dict(order=odd8), dict(starts=odd8), dict(grad=odd), dict(chan=524281)):
        assert d_other(**kw) == -3, kw
    # the keys are 63-bit: a batch whose keys would not fit is refused
    assert fwd(n=65535, h=32768, w=32768, hl=32768, wl=32768, out_bs=81 * (1 << 30)) == -3
