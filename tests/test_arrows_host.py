"""CPU tier of Flow.visualise_arrows / visualise_flow_arrows: the oracle (tests/arrows_oracle.py) pinned by hand-computed
cases (the rasteriser of DESIGN.md 3.11, the grid, the painter's order, the 's' thickness quirk, the batch-wide scaling), the host
logic of the API with the native calls served by the oracle, and the C ABI's argument checks."""
import ctypes
import math

import numpy as np
import pytest
import torch

import arrows_oracle as ao
import vis_oracle as vo

TINY = 1e-12        # a tip length that folds both barbs into the tip: the shaft alone
WHITE, BLACK = 255, (0, 0, 0)


def _canvas(h=40, w=60):
    return np.full((h, w, 3), WHITE, np.uint8)


def _grey(alpha):
    """a black arrow over white at coverage alpha"""
    return int(np.rint(255.0 + alpha * (0.0 - 255.0)))


# ---- the rasteriser ---------------------------------------------------------------------------------------------------------------
def test_prototype_arrow():
    p1, p2 = (10, 10), (45, 28)
    tip = 3.5 / math.hypot(35, 18)
    assert ao.barbs(p1, p2, tip) == ((44, 25), (42, 29))
    img = _canvas(40, 60)
    ao.draw_arrow(img, p1, p2, BLACK, 1, tip)
    assert all(tuple(img[y, x]) == BLACK for x, y in (p1, p2, (44, 25), (42, 29)))         # alpha 1 at every end
    touched = (img != WHITE).any(-1)
    # a clean one-pixel line: the band |d| < 1 is 2 / cos(slope) = 2.25 pixels high, so two or three pixel centres per column
    assert touched[:, 10:40].sum(0).max() <= 3 and touched[:, 10:40].sum(0).min() >= 2
    assert not touched[:, :9].any() and not touched[:, 47:].any() and not touched[:9].any() and not touched[31:].any()


@pytest.mark.parametrize("t", [1, 2, 3])
def test_horizontal_and_vertical_shaft_coverage(t):
    for vertical in (False, True):
        img = _canvas()
        a, b = ((20, 5), (20, 30)) if vertical else ((10, 20), (40, 20))
        ao.draw_arrow(img, a, b, BLACK, t, TINY)
        view = img.transpose(1, 0, 2) if vertical else img          # view[across, along]
        along, across = (5, 30, 20) if vertical else (10, 40, 20), None
        lo, hi, axis = along
        for d in range(0, 5):                                        # alpha = clamp(t / 2 + 0.5 - d, 0, 1)
            alpha = min(max(t / 2 + 0.5 - d, 0.0), 1.0)
            for sgn in (-1, 1):
                assert np.all(view[axis + sgn * d, lo:hi + 1] == _grey(alpha)), (t, d)
        if t == 2:
            assert _grey(0.5) == 128 and np.all(view[axis + 1, lo:hi + 1] == 128)      # 0.5 at distance t / 2, half to even
        # round caps: beyond the end the distance is to the end point
        for d in range(1, 5):
            alpha = min(max(t / 2 + 0.5 - d, 0.0), 1.0)
            assert np.all(view[axis, hi + d] == _grey(alpha)) and np.all(view[axis, lo - d] == _grey(alpha))
        first_clear = int(math.ceil(t / 2 + 0.5))
        assert np.all(view[axis + first_clear] == WHITE) and np.all(view[:, hi + first_clear] == WHITE)


@pytest.mark.parametrize("t", [1, 3])
def test_diagonal_shaft_coverage(t):
    img = _canvas()
    ao.draw_arrow(img, (10, 5), (35, 30), BLACK, t, TINY)
    r = t / 2 + 0.5
    for k in range(0, 5):                                            # (x + k, y) lies k / sqrt(2) from the line
        d2 = np.float64(k * k * 25 * 25) / np.float64(2 * 25 * 25)   # cross^2 / L2, as the definition forms it
        alpha = min(max(r - float(np.sqrt(d2)), 0.0), 1.0)
        for s in range(3, 22):
            assert np.all(img[5 + s, 10 + s + k] == _grey(alpha)) and np.all(img[5 + s + k, 10 + s] == _grey(alpha)), (t, k)
    assert _grey(1 - 1 / math.sqrt(2)) == 180 and (t != 1 or np.all(img[15, 21] == 180))


def test_zero_length_arrow_is_a_disc():
    for t, ring, diag in ((1, 0.0, 0.0), (3, 1.0, 2 - math.sqrt(2))):
        img = _canvas()
        ao.draw_arrow(img, (30, 20), (30, 20), (10, 20, 30), t, 0.7)
        assert tuple(img[20, 30]) == (10, 20, 30)
        for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            assert tuple(img[20 + dy, 30 + dx]) == tuple(int(np.rint(255 + ring * (c - 255))) for c in (10, 20, 30))
        assert tuple(img[21, 31]) == tuple(int(np.rint(255.0 + diag * (c - 255.0))) for c in (10, 20, 30))
        assert np.all(img[20, 33:] == WHITE) and np.all(img[23:] == WHITE)


def test_arrow_leaving_the_frame_is_clipped():
    img = _canvas()
    ao.draw_arrow(img, (50, 20), (100, 20), BLACK, 1, TINY)
    assert np.all(img[20, 50:] == 0) and np.all(img[20, :49] == WHITE) and np.all(img[19] == WHITE)
    before = img.copy()
    ao.draw_arrow(img, (70, -30), (200, -90), BLACK, 3, 0.1)                 # wholly outside: nothing happens
    ao.draw_arrow(img, (-2 ** 20, 5), (-2 ** 19, 5), BLACK, 3, 0.1)
    assert np.array_equal(img, before)
    ao.draw_arrow(img, (-2 ** 20, 5), (2 ** 20, 5), (1, 2, 3), 1, TINY)      # far ends, exact integers: the whole row
    assert np.all(img[5] == (1, 2, 3)) and np.all(img[4] == WHITE) and np.all(img[6] == WHITE)


def test_crossing_arrows_later_on_top():
    img = _canvas()
    ao.draw_arrow(img, (10, 20), (50, 20), (200, 0, 0), 1, TINY)
    ao.draw_arrow(img, (30, 5), (30, 35), (0, 200, 0), 1, TINY)
    assert tuple(img[20, 30]) == (0, 200, 0) and tuple(img[20, 29]) == (200, 0, 0) and tuple(img[19, 30]) == (0, 200, 0)
    # one blend per arrow and pixel: where shaft and barbs overlap near the tip the pixel is blended once
    a, b = _canvas(), _canvas()
    ao.draw_arrow(a, (10, 20), (40, 20), BLACK, 2, 0.3)
    for seg in (((10, 20), (40, 20)),) + tuple((bb, (40, 20)) for bb in ao.barbs((10, 20), (40, 20), 0.3)):
        ao.draw_arrow(b, seg[0], seg[1], BLACK, 2, TINY)
    assert np.all(a >= b) and (a > b).any()


def test_hue_table():
    assert ao.HUES.shape == (181, 3) and ao.HUES.dtype == np.uint8
    assert tuple(ao.HUES[0]) == (0, 0, 255) and tuple(ao.HUES[60]) == (0, 255, 0) and tuple(ao.HUES[120]) == (255, 0, 0)
    assert tuple(ao.HUES[180]) == (0, 0, 255) and tuple(ao.HUES[30]) == (0, 255, 255)
    # the colour Flow.visualise('bgr') paints for that hue at full saturation
    f = np.zeros((1, 2, 1, 4), np.float32)
    f[0, 0], f[0, 1] = [1, 0, -1, 0], [0, 1, 0, -1]
    vis = vo.visualise(f, 'bgr', range_max=np.array([1.0]))[0, 0]
    assert [tuple(v) for v in vis] == [tuple(ao.HUES[h]) for h in (0, 45, 90, 135)]


# ---- the grid, the order, the reference's quirks ------------------------------------------------------------------------------------
def test_grid_counts_positions_and_reset():
    pts = ao.grid_points(100, 150, 20)
    assert pts.dtype == np.int32 and len(pts) == 5 * 7
    assert [int(v) for v in pts[:8, 1]] == [10, 30, 50, 70, 90, 110, 130, 10] and [int(v) for v in pts[::7, 0]] == [10, 30, 50, 70, 90]
    assert [tuple(p) for p in ao.grid_points(21, 41, 10)] == [(5, 5), (5, 15), (5, 25), (5, 35), (15, 5), (15, 15), (15, 25), (15, 35)]
    assert [tuple(p) for p in ao.grid_points(20, 11, 10)] == [(5, 5), (15, 5)]      # end exclusive: rows below 19, columns below 10
    assert ao.effective_grid_dist(11, 30, None) == 5 and ao.effective_grid_dist(11, 30, 7) == 5 and ao.effective_grid_dist(11, 30, 3) == 3
    assert [tuple(p) for p in ao.grid_points(11, 11, 5)] == [(2, 2), (2, 7), (7, 2), (7, 7)]
    assert [tuple(p) for p in ao.grid_points(2, 2, 1)] == [(0, 0)] and len(ao.grid_points(2, 3, 1)) == 2
    out = ao.visualise_arrows(np.zeros((2, 2, 11, 30), np.float32), 't', grid_dist=None)            # reset to 5, red pixels only
    red = (out == (0, 0, 255)).all(-1)
    assert red.sum() == 2 * 2 * 6 and (out[~red] == WHITE).all() and red[1, 7, 27] and red[0, 2, 2]


def _translation(n, h, w, dx, dy):
    f = np.zeros((n, 2, h, w), np.float32)
    f[:, 0], f[:, 1] = np.float32(dx), np.float32(dy)
    return f


def test_painters_order_and_red_pixels():
    h, w, g = 30, 60, 10
    pts = ao.grid_points(h, w, g)
    # 's', +10 px: every arrow ends on the NEXT grid point, whose red pixel is painted later -> every grid pixel is red
    out = ao.visualise_arrows(_translation(1, h, w, 10, 0), 's', grid_dist=g, scaling=1)[0]
    assert all(tuple(out[y, x]) == (0, 0, 255) for y, x in pts)
    assert tuple(out[5, 10]) == tuple(ao.HUES[0])                        # the arrow between them, in the hue of 0 degrees
    # 's', -10 px: every arrow ends on the PREVIOUS grid point and paints over its (earlier) red pixel
    out = ao.visualise_arrows(_translation(1, h, w, -10, 0), 's', grid_dist=g, scaling=1)[0]
    col = tuple(ao.HUES[90])
    for y, x in pts:
        last_of_row = x == pts[:, 1].max()
        assert tuple(out[y, x]) == ((0, 0, 255) if last_of_row else col)
    # 't', +10 px: arrow j runs from the previous grid point to point j: the previous red pixel is covered, its own is not
    out = ao.visualise_arrows(_translation(1, h, w, 10, 0), 't', grid_dist=g, scaling=1)[0]
    for y, x in pts:
        assert tuple(out[y, x]) == ((0, 0, 255) if x == pts[:, 1].max() else tuple(ao.HUES[0]))
    # below the drawing threshold nothing but the red pixels
    out = ao.visualise_arrows(_translation(1, h, w, 0.5, 0), 's', grid_dist=g, scaling=1)[0]
    assert ((out != WHITE).any(-1)).sum() == len(pts)
    out = ao.visualise_arrows(_translation(1, h, w, 0.51, 0), 's', grid_dist=g, scaling=1)[0]
    assert ((out != WHITE).any(-1)).sum() > len(pts)


def test_s_ignores_thickness_for_the_line_but_not_for_the_tip():
    h, w, g = 40, 80, 20
    f = _translation(1, h, w, 30, 0)
    s1 = ao.visualise_arrows(f, 's', grid_dist=g, scaling=1, thickness=1, colour=BLACK)[0]
    s6 = ao.visualise_arrows(f, 's', grid_dist=g, scaling=1, thickness=6, colour=BLACK)[0]
    t6 = ao.visualise_arrows(f, 't', grid_dist=g, scaling=1, thickness=6, colour=BLACK)[0]
    # mid-shaft of the first arrow (10, 10) -> (40, 10): two rows off the axis
    assert np.all(s1[12, 20] == WHITE) and np.all(s6[12, 20] == WHITE) and np.all(s6[10, 20] == 0)
    assert not np.array_equal(s1, s6)                                      # the tip is sized by sqrt(6) * 3.5
    manual = np.full((h, w, 3), WHITE, np.uint8)
    for y, x in ao.grid_points(h, w, g):
        ao.draw_arrow(manual, (int(x), int(y)), (int(x) + 30, int(y)), BLACK, 1, float(math.sqrt(6) * 3.5 / np.float32(30)))
        manual[y, x] = (0, 0, 255)
    assert np.array_equal(s6, manual)
    # 't' honours it: alpha 1 up to t / 2 - 0.5 = 2.5 from the axis, 0.5 at 3 (column 15: the arrow (0, 10) -> (30, 10) alone)
    assert np.all(t6[12, 15] == 0) and np.all(t6[13, 15] == 128) and np.all(t6[14, 15] == WHITE)


def test_scaling_is_grid_dist_over_numpy_percentile():
    rs = np.random.RandomState(3)
    vecs = (rs.randn(3, 2, 50, 70) * 4).astype(np.float32)
    vecs[:, :, :10, :10] = 5e-4                                           # thresholded to zero
    for g in (3, 10):
        ys, xs = np.arange(g // 2, 49, g), np.arange(g // 2, 69, g)
        sub = vecs[:, :, ys][:, :, :, xs]
        mags, _ = vo.cart_to_polar(vo.threshold(sub[:, 0]), vo.threshold(sub[:, 1]))
        direct = g / np.percentile(mags.reshape(3, -1), 99)                # ONE scalar for the batch
        _, used = ao.visualise_arrows(vecs, 't', grid_dist=g, return_scaling=True)
        assert isinstance(used, np.float32) and used.view(np.uint32) == direct.view(np.uint32)
        assert np.float32(np.float32(g) / vo.percentile_lerp(mags)).view(np.uint32) == used.view(np.uint32)
        per_image = [g / np.percentile(mags[i], 99) for i in range(3)]
        assert not any(p == used for p in per_image)


# ---- host logic: the API with the native calls served by the oracle ----------------------------------------------------------------
def _fake_scale(vecs, grid_dist):
    _, _, mags, _ = ao.sample(vecs.detach().cpu().float().numpy(), grid_dist)
    return torch.from_numpy(np.array([ao.default_scaling(mags, grid_dist)], np.float32))


def _fake_arrows(vecs, ref, grid_dist, scaling, thickness, colour=None, img=None, img_interleaved=False, mask=None,
                 show_mask=False, show_mask_borders=False, layout=0):
    v = vecs.detach().cpu().float().numpy()
    s = np.float32(scaling.item()) if isinstance(scaling, torch.Tensor) else scaling
    bg = None if img is None else (img.cpu().numpy() if img_interleaved else np.moveaxis(img.cpu().numpy(), 1, -1))
    out = ao.visualise_arrows(v, ref, None if mask is None else mask.cpu().numpy(), grid_dist, bg, s, show_mask, show_mask_borders,
                              colour, thickness)
    return torch.from_numpy(out if layout == 1 else np.ascontiguousarray(np.moveaxis(out, -1, 1)))


@pytest.fixture
def arrows_native(oracle_native, monkeypatch):
    from oflibpytorch_amd import _native
    monkeypatch.setattr(_native, "arrows_scale", _fake_scale)
    monkeypatch.setattr(_native, "arrows", _fake_arrows)
    return _native


def _reference_test_flows(ofl, ref):
    h, w = 64, 80
    mask = np.zeros((h, w))
    mask[20:-20, 10:-10] = 1
    flow1 = ofl.batch_flows((ofl.Flow.from_transforms([['translation', 10, -8]], (h, w), ref, mask),
                             ofl.Flow.from_transforms([['translation', -5, 10]], (h, w), ref, mask),
                             ofl.Flow.from_transforms([['rotation', 30, 50, 30]], (h, w), ref, mask)))
    return flow1, mask


def test_host_errors_of_the_reference_test(arrows_native):
    """test/test_flow_class.py:1844-1875 of the reference: the same classes, with its messages"""
    import oflibpytorch_amd as ofl
    flow1, mask = _reference_test_flows(ofl, 't')
    img_np = np.random.RandomState(1).randint(0, 256, (64, 80, 3)).astype(np.uint8)
    img_np_3 = np.broadcast_to(img_np, (3, *img_np.shape)).copy()
    with pytest.raises(TypeError, match="Grid_dist needs to be an integer value"):
        flow1.visualise_arrows(grid_dist='test')
    with pytest.raises(ValueError, match="Grid_dist needs to be an integer larger than zero"):
        flow1.visualise_arrows(grid_dist=-1)
    with pytest.raises(TypeError, match="Img needs to be a numpy array or a torch tensor"):
        flow1.visualise_arrows(10, img='test')
    for bad in (mask, mask[10:], img_np[..., :2], img_np_3[:2]):
        with pytest.raises(ValueError, match="Img needs to have 3 or 4 channels and the same shape as the flow"):
            flow1.visualise_arrows(10, img=bad)
    with pytest.raises(TypeError, match="Scaling needs to be a float or an integer"):
        flow1.visualise_arrows(10, img_np, scaling='test')
    with pytest.raises(ValueError, match="Scaling needs to be larger than zero"):
        flow1.visualise_arrows(10, img_np, scaling=-1)
    with pytest.raises(TypeError, match="Show_mask needs to be boolean"):
        flow1.visualise_arrows(10, img_np, None, show_mask='test')
    with pytest.raises(TypeError, match="Show_mask_borders needs to be boolean"):
        flow1.visualise_arrows(10, img_np, None, True, show_mask_borders='test')
    with pytest.raises(TypeError, match="Colour needs to be a tuple"):
        flow1.visualise_arrows(10, img_np, None, True, True, colour='test')
    with pytest.raises(ValueError, match="Colour list or tuple needs to have length 3"):
        flow1.visualise_arrows(10, img_np, None, True, True, colour=(0, 0))
    with pytest.raises(TypeError, match="Return_tensor needs to be boolean"):
        flow1.visualise_arrows(10, img_np, None, True, True, colour=(0, 0, 0), return_tensor='test')
    with pytest.raises(TypeError, match="Thickness needs to be an integer"):
        flow1.visualise_arrows(thickness=0.5)
    with pytest.raises(ValueError, match="Thickness needs to be a integer larger than zero"):
        flow1.visualise_arrows(thickness=0)
    # the reference's order: grid_dist before img before scaling before the booleans before colour before thickness
    with pytest.raises(TypeError, match="Grid_dist"):
        flow1.visualise_arrows('x', img='test', thickness=0)
    with pytest.raises(TypeError, match="Img needs to be a numpy"):
        flow1.visualise_arrows(10, img='test', scaling='x')
    with pytest.raises(TypeError, match="Scaling"):
        flow1.visualise_arrows(10, img_np, scaling='x', show_mask=3)
    with pytest.raises(TypeError, match="Show_mask needs"):
        flow1.visualise_arrows(10, img_np, show_mask=3, colour='x')
    with pytest.raises(TypeError, match="Colour"):
        flow1.visualise_arrows(10, img_np, colour='x', thickness=0)
    # this package's own check: uint8 only
    with pytest.raises(TypeError, match="Img needs to be of dtype uint8"):
        flow1.visualise_arrows(10, img_np.astype(np.float32))
    with pytest.raises(TypeError, match="Img needs to be of dtype uint8"):
        flow1.visualise_arrows(10, torch.zeros(3, 64, 80))
    with pytest.raises(ImportError if not hasattr(ofl, 'visualise_flow_arrows') else ValueError):
        ofl.visualise_flow_arrows(flow1.vecs, 't', grid_dist=0)


def test_host_reference_test_loop_types_and_values(arrows_native):
    """the loop of test/test_flow_class.py:1797-1843 (types), with the values checked against the oracle called directly"""
    import oflibpytorch_amd as ofl
    img_np = np.random.RandomState(2).randint(0, 256, (64, 80, 3)).astype(np.uint8)
    img_pt = torch.tensor(img_np).permute(2, 0, 1)
    forms = [None, img_np, img_pt, img_np[np.newaxis], img_pt.unsqueeze(0), np.broadcast_to(img_np, (3, 64, 80, 3)).copy(),
             img_pt.unsqueeze(0).expand(3, -1, -1, -1)]
    for ref in ('s', 't'):
        flow1, _ = _reference_test_flows(ofl, ref)
        v, m = flow1.vecs.numpy(), flow1.mask.numpy()
        for scaling, show_mask, borders in ((0.1, True, False), (1, False, True), (2, True, True), (None, False, False)):
            for img in forms:
                keep = None if img is None else (img.copy() if isinstance(img, np.ndarray) else img.clone())
                exp = ao.visualise_arrows(v, ref, m, 10, None if img is None else img_np, scaling, show_mask, borders)
                t = flow1.visualise_arrows(grid_dist=10, scaling=scaling, img=img, show_mask=show_mask, show_mask_borders=borders,
                                           return_tensor=True)
                a = flow1.visualise_arrows(grid_dist=10, scaling=scaling, img=img, show_mask=show_mask, show_mask_borders=borders,
                                           return_tensor=False)
                assert isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.shape == (3, 3, 64, 80)
                assert isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.shape == (3, 64, 80, 3)
                assert np.array_equal(a, exp) and np.array_equal(np.moveaxis(t.numpy(), 1, -1), exp)
                if img is not None:                                       # the caller's image is never written to
                    assert np.array_equal(img, keep) if isinstance(img, np.ndarray) else torch.equal(img, keep)
        for colour in (None, (100, 100, 100), (300.0, -4, 99.5)):         # (saturated like an OpenCV scalar: 255, 0, 100)
            got = flow1.visualise_arrows(10, img_np, 1, colour=colour, thickness=2, return_tensor=False)
            sat = None if colour is None else tuple(int(c) for c in np.clip(np.rint(colour), 0, 255))
            assert np.array_equal(got, ao.visualise_arrows(v, ref, m, 10, img_np, 1, colour=sat, thickness=2))


def test_host_grid_dist_reset_warning_and_squeeze(arrows_native, capsys):
    import oflibpytorch_amd as ofl
    f = torch.randn(2, 11, 30, 2)          # channel-last, as the reference accepts
    fl = ofl.Flow(f, 's')
    out = fl.visualise_arrows()
    printed = capsys.readouterr().out
    assert "Warning: grid_dist in visualise_arrows is '20', which is too large for a flow field of shape (11, 30). " \
           "grid_dist will be reset to '5'." in printed
    assert out.shape == (2, 3, 11, 30)
    assert np.array_equal(np.moveaxis(out.numpy(), 1, -1), ao.visualise_arrows(fl.vecs.numpy(), 's', grid_dist=5))
    fl.visualise_arrows(5)
    assert capsys.readouterr().out == ""
    bg = np.full((11, 30, 3), 7, np.uint8)
    a3 = ofl.visualise_flow_arrows(f[0], 's', 5, bg, 1.5, (1, 2, 3), 2)
    assert isinstance(a3, torch.Tensor) and a3.shape == (3, 11, 30)
    assert torch.equal(a3, fl.visualise_arrows(5, bg, 1.5, colour=(1, 2, 3), thickness=2)[0])
    n3 = ofl.visualise_flow_arrows(f[0].numpy(), 's', 5, return_tensor=False)
    assert isinstance(n3, np.ndarray) and n3.shape == (11, 30, 3)
    assert ofl.visualise_flow_arrows(f, 't', 5, return_tensor=False).shape == (2, 11, 30, 3)
    with pytest.raises(ValueError, match="Grid_dist needs to be an integer larger than zero"):
        ofl.Flow(torch.zeros(1, 2, 1, 9)).visualise_arrows()             # min(H, W) // 2 = 0
    with pytest.raises(ValueError, match="Error visualising flow arrows: "):
        bad = ofl.Flow(torch.zeros(1, 2, 8, 8))
        bad.vecs[0, 0, 0, 0] = float('nan')
        bad.visualise_arrows(2)


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
def test_cabi_arrows_rejects_bad_arguments():
    from oflibpytorch_amd import _native
    lib = _native.load_library()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)    # (never dereferenced: rejected before any launch)
    ints = lib.ofl_arrows_workspace_ints
    assert ints(0, 8, 8, 2) == -2 and ints(1, 1, 8, 1) == -2 and ints(70000, 8, 8, 2) == -2
    assert ints(1, 8, 8, 0) == -3 and ints(1, 8, 9, 5) == -3 and ints(1, 8, 9, 4) > 0
    # header | two int64 per image | n * P magnitudes | n * P records | three words per tile
    assert ints(2, 1080, 1920, 20) == 16 + 4 * 2 + 2 * 54 * 96 * (1 + 20) + 3 * 2 * 30 * 68
    sc = lib.ofl_arrows_scale_f32
    assert sc(null, 0, 0, 2, one, one, 1, 8, 8, null) == -1 and sc(one, 0, 0, 2, null, one, 1, 8, 8, null) == -1
    assert sc(one, 0, 0, 2, one, null, 1, 8, 8, null) == -1
    assert sc(one, 0, 0, 2, one, one, 0, 8, 8, null) == -2 and sc(one, 0, 0, 5, one, one, 1, 8, 8, null) == -3
    assert sc(one, 0, 2, 2, one, one, 1, 8, 8, null) == -3 and sc(one, -1, 0, 2, one, one, 1, 8, 8, null) == -3
    plan = lib.ofl_arrows_plan
    assert plan(null, 0, 0, 0, 2, one, -1, 1, 3.5, one, 1, 8, 8, null) == -1
    assert plan(one, 0, 0, 0, 2, null, -1, 1, 3.5, one, 1, 8, 8, null) == -1
    assert plan(one, 0, 0, 0, 2, one, -1, 1, 3.5, null, 1, 8, 8, null) == -1
    assert plan(one, 0, 0, 0, 2, one, -1, 1, 3.5, one, 1, 8, 1, null) == -2
    assert plan(one, 0, 0, 2, 2, one, -1, 1, 3.5, one, 1, 8, 8, null) == -3          # ref
    assert plan(one, 0, 0, 0, 2, one, -1, 0, 3.5, one, 1, 8, 8, null) == -3          # thickness
    assert plan(one, 0, 0, 0, 2, one, -1, 40000, 3.5, one, 1, 8, 8, null) == -3
    assert plan(one, 0, 0, 0, 2, one, 1 << 24, 1, 3.5, one, 1, 8, 8, null) == -3     # colour
    assert plan(one, 0, 0, 0, 2, one, -1, 1, 0.0, one, 1, 8, 8, null) == -3          # tip size
    u8 = lib.ofl_arrows_u8
    assert u8(null, 0, 0, null, 0, 0, 0, 2, null, one, 4, 0, one, 1, 8, 8, null) == -1
    assert u8(null, 0, 0, null, 0, 0, 0, 2, one, one, 4, 0, null, 1, 8, 8, null) == -1
    assert u8(null, 0, 0, null, 0, 0, 0, 2, one, null, 4, 0, one, 1, 8, 8, null) == -1
    assert u8(null, 0, 0, null, 0, 0, 0, 2, one, one, 4, 0, one, 1, 8, 0, null) == -2
    assert u8(null, 0, 0, null, 0, 0, 0, 9, one, one, 4, 0, one, 1, 8, 8, null) == -3
    assert u8(null, 0, 0, null, 0, 0, 0, 2, one, one, 4, 2, one, 1, 8, 8, null) == -3
    assert u8(null, 0, 2, null, 0, 0, 0, 2, one, one, 4, 0, one, 1, 8, 8, null) == -3
    assert u8(null, 0, 0, null, 0, 2, 0, 2, one, one, 4, 0, one, 1, 8, 8, null) == -3
    assert u8(null, 0, 0, null, 0, 0, 3, 2, one, one, 4, 0, one, 1, 8, 8, null) == -3
    assert u8(null, 0, 0, null, 0, 0, 0, 2, one, one, -4, 0, one, 1, 8, 8, null) == -3
