"""CPU tier of the triangle-mesh interpolator: the NumPy restatement tests/mesh_oracle.py against
scipy.interpolate.griddata called exactly as the reference calls it (utils.py:577-600, :1020-1032), hand-built cases for each rule of
the definition, and the contract of the public switch.  The HIP kernels are held to the same oracle in tests/test_gpu_mesh.py."""
import numpy as np
import pytest
import torch

import mesh_oracle as mo
import oflibpytorch_amd as ofl
from oflibpytorch_amd import Flow

scipy_interpolate = pytest.importorskip("scipy.interpolate")

# |mesh - griddata| wherever both define a pixel: the largest difference measured over every case below is 4.5e-16 for data in
# [0, 1) and 8.6e-14 for data in [0, 255) (SciPy 1.15.3; float64 rounding of two different but equivalent barycentric formulas);
# the bound is 100 x that, relative to the data's scale.
TOL_UNIT = 4.5e-14
SIZES = [(40, 56), (33, 47), (25, 61)]
SEEDS = [0, 1, 2]


def smooth_flow(h, w, seed, maxdiff=0.25):
    """A few low-frequency sinusoids per component, scaled so that the largest neighbour-to-neighbour difference is `maxdiff`"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    f = np.zeros((2, h, w))
    for c in range(2):
        for _ in range(4):
            kx, ky = rng.uniform(-1, 1, 2) * 2 * np.pi / max(h, w) * 5.0
            f[c] += rng.uniform(0.5, 1.5) * np.sin(kx * xx + ky * yy + rng.uniform(0, 2 * np.pi))
    d = max(np.abs(np.diff(f, axis=1)).max(), np.abs(np.diff(f, axis=2)).max())
    return (f * (maxdiff / d)).astype(np.float32)


def griddata_apply(flow, data):
    """utils.py:579-599 for one batch member: -> float64 [C,H,W], NaN outside the convex hull"""
    h, w = flow.shape[1:]
    field = np.moveaxis(flow, 0, -1).astype('float32')
    flow_flat = np.reshape(field[..., ::-1], (-1, 2))
    x, y = np.mgrid[:h, :w]
    positions = np.swapaxes(np.vstack([x.ravel(), y.ravel()]), 0, 1)
    pos = positions + flow_flat
    target_flat = np.reshape(np.moveaxis(data, 0, -1), (-1, data.shape[0]))
    return np.moveaxis(scipy_interpolate.griddata(pos, target_flat, (x, y), method='linear'), -1, 0)


def griddata_track(flow, pts):
    """utils.py:1021-1031 for one batch member: -> float64 [M,2] (y, x) flow vectors, NaN outside the convex hull"""
    h, w = flow.shape[1:]
    fl = np.moveaxis(flow, 0, -1).astype('float32')
    flow_flat = np.reshape(fl[..., ::-1], (-1, 2))
    x, y = np.mgrid[:h, :w]
    grid = np.swapaxes(np.vstack([x.ravel(), y.ravel()]), 0, 1)
    origin_points = grid - flow_flat
    return scipy_interpolate.griddata(origin_points, flow_flat, (pts[:, 0], pts[:, 1]), method='linear')


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("integer", [False, True])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("size", SIZES)
def test_oracle_equals_griddata_on_smooth_flows(size, seed, integer, c):
    h, w = size
    flow = smooth_flow(h, w, seed)
    assert max(np.abs(np.diff(flow, axis=1)).max(), np.abs(np.diff(flow, axis=2)).max()) <= 0.2500001
    rng = np.random.default_rng(100 + seed)
    if integer:
        data = rng.integers(0, 256, (c, h, w)).astype(np.uint8)
    else:
        data = rng.uniform(0, 1, (c, h, w)).astype(np.float32)
    ref = griddata_apply(flow, data)
    raw, inside, _ = mo.mesh_apply(flow, data, raw=True)
    fin, ins = np.isfinite(ref).all(axis=0), inside.astype(bool)
    both = fin & ins
    err = np.abs(ref - raw)[:, both].max()
    left_out = fin & ~ins
    print("size %s seed %d c %d integer %d: max |mesh - griddata| %.3g, left out %.2f %%"
          % (size, seed, c, integer, err, 100.0 * left_out.mean()))
    assert err <= TOL_UNIT * (255.0 if integer else 1.0)
    assert not (ins & ~fin).any()                        # the mesh defines no pixel griddata leaves NaN
    assert left_out.mean() <= 0.05
    # ... and only in the band the displaced image's border can reach
    band = int(np.ceil(np.abs(flow).max())) + 1
    yy, xx = np.nonzero(left_out)
    assert all(min(y, x, h - 1 - y, w - 1 - x) <= band for y, x in zip(yy, xx))
    if integer:
        # after the reference's rounding (utils.py:612-618) both give the same integers, bar values that sit on a .5 boundary
        out = mo.mesh_apply(flow, data, round_mode=mo.ROUND_U8)[0]
        want = np.clip(np.rint(np.nan_to_num(ref).astype(np.float32)), 0, 255).astype(np.uint8)
        tie = np.abs(np.abs(ref - np.floor(ref)) - 0.5) < 1e-4
        assert out.dtype == np.uint8 and np.array_equal(out[:, both][~tie[:, both]], want[:, both][~tie[:, both]])


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("size", SIZES)
def test_oracle_point_query_equals_griddata(size, seed):
    h, w = size
    flow = smooth_flow(h, w, seed)
    rng = np.random.default_rng(200 + seed)
    pts = np.stack([rng.uniform(0, h - 1, 300), rng.uniform(0, w - 1, 300)], axis=1).astype(np.float32)
    pts[:20] = np.round(pts[:20])                        # some on pixel centres
    ref = griddata_track(flow, pts)
    vecs, inside = mo.mesh_points(flow, pts)
    fin, ins = np.isfinite(ref).all(axis=1), inside.astype(bool)
    both = fin & ins
    err = np.abs(ref - vecs)[both].max()
    left_out = fin & ~ins
    print("size %s seed %d: max |mesh - griddata| %.3g over %d points, left out %.2f %%" % (size, seed, err, both.sum(), 100.0 * left_out.mean()))
    assert err <= TOL_UNIT * max(1.0, float(np.abs(flow).max()))
    assert not (ins & ~fin).any()
    assert left_out.mean() <= 0.05
    band = int(np.ceil(np.abs(flow).max())) + 1
    assert all(min(y, x, h - 1 - y, w - 1 - x) <= band for y, x in pts[left_out])
    moved = mo.track(flow, pts)
    assert moved.dtype == np.float32 and np.array_equal(moved[~ins], np.zeros_like(moved[~ins]))


# ---- the rules of the definition, one by one --------------------------------------------------------------------------------------
def _ramp(c, h, w):
    return (np.arange(c * h * w, dtype=np.float32).reshape(c, h, w) % 251) / 8


def test_tie_rule_keeps_the_main_diagonal_on_an_identity_flow():
    """every quad of an undisplaced grid is co-circular: the split is A-C ((i, j)-(i+1, j+1)), the interpolation the identity"""
    h, w = 6, 7
    flow = np.zeros((2, h, w), np.float32)
    vx, vy, usable = mo.vertices(flow)
    tr = mo.triangles(vx, vy, usable)
    assert not tr['bd'].any() and tr['valid'].all()
    assert tr['src'][0].tolist() == [0, 1, w + 1] and tr['src'][1].tolist() == [0, w + 1, w]
    data = _ramp(2, h, w)
    out, inside, owner = mo.mesh_apply(flow, data)
    assert inside.all() and np.array_equal(out, data)
    # a pixel is a vertex of up to six triangles: the lowest number wins -- quad (i-1, j-1)'s triangle 0 ... for the inner ones
    assert owner[0, 0] == 0 and owner[1, 1] == 0 and owner[0, 1] == 0 and owner[1, 0] == 1 and owner[2, 2] == 2 * (1 * (w - 1) + 1)
    # a constant shift is the same tie, moved: still A-C
    tr = mo.triangles(*mo.vertices(flow + np.float32(0.375)))
    assert not tr['bd'].any()


def test_in_circle_test_picks_the_other_diagonal():
    h, w = 2, 2
    flow = np.zeros((2, h, w), np.float32)
    flow[:, 1, 0] = (0.25, -0.25)                         # D moves towards B: inside the circle through A, B, C
    tr = mo.triangles(*mo.vertices(flow))
    assert tr['bd'].all() and tr['src'][0].tolist() == [0, 1, 2] and tr['src'][1].tolist() == [1, 3, 2]
    flow[:, 1, 0] = (-0.25, 0.25)                         # ... away from it: outside, A-C stays
    assert not mo.triangles(*mo.vertices(flow))['bd'].any()


def test_masked_vertex_removes_its_quads_and_three_usable_vertices_give_no_triangle():
    h, w = 6, 6
    flow = np.full((2, h, w), 0.25, np.float32)
    mask = np.ones((h, w), bool)
    mask[3, 2] = False
    out, inside, owner = mo.mesh_apply(flow, _ramp(1, h, w), mask=mask)
    tr = mo.triangles(*mo.vertices(flow, mask=mask))
    gone = {2 * (i * (w - 1) + j) + k for i in (2, 3) for j in (1, 2) for k in (0, 1)}
    assert set(np.flatnonzero(~tr['valid']).tolist()) == gone
    # the pixels strictly inside the hole of the four quads (shifted by 0.25) are outside every triangle and give 0
    assert inside[3, 3] == 0 and inside[4, 3] == 0 and inside[3, 2] == 0 and out[0, 3, 3] == 0
    assert inside[2, 2] == 1 and inside[5, 5] == 1 and inside[0, 0] == 0
    # a non-finite vertex does the same
    bad = flow.copy()
    bad[0, 3, 2] = np.inf
    assert np.array_equal(mo.mesh_apply(bad, _ramp(1, h, w))[1], inside)


def test_fold_lower_numbered_triangle_wins():
    h, w = 4, 8
    flow = np.zeros((2, h, w), np.float32)
    flow[0, :, 4:] = -3.0                                 # columns 4.. land on columns 1..: the sheet folds back over itself
    data = _ramp(1, h, w)
    out, inside, owner = mo.mesh_apply(flow, data)
    # pixel (1, 2) lies in the unmoved quads of column 1-2 (lower numbers) and in the moved ones of columns 4-5
    assert owner[1, 2] == 2 * (0 * (w - 1) + 1) and out[0, 1, 2] == data[0, 1, 2]
    assert owner[2, 3] == 2 * (1 * (w - 1) + 2) and out[0, 2, 3] == data[0, 2, 3]
    assert inside[:, 5:].sum() == 0 and inside[:, :5].all()


def test_degenerate_triangles_are_dropped():
    h, w = 3, 3
    flow = np.zeros((2, h, w), np.float32)
    flow[0, :, 1] = 1.0                                   # column 1 lands on column 2: the quads between them have no area
    tr = mo.triangles(*mo.vertices(flow))
    assert tr['valid'].tolist() == [True, True, False, False, True, True, False, False]
    out, inside, _ = mo.mesh_apply(flow, _ramp(1, h, w))
    assert inside[:, 0].all() and inside[:, 2].all()


def test_query_on_an_edge_and_on_a_vertex_is_inside():
    h, w = 3, 3
    flow = np.zeros((2, h, w), np.float32)
    data = _ramp(1, h, w)
    pts = np.array([[1.0, 1.0], [0.5, 0.5], [0.0, 0.5], [2.0, 2.0], [1.5, 1.0], [0.25, 0.75]])
    vecs, inside = mo.mesh_points(flow + np.float32(0.0), pts)
    assert inside.all() and np.array_equal(vecs, np.zeros_like(vecs))
    tr = mo.triangles(*mo.vertices(flow))
    owner = mo.point_owners(tr, pts, h, w)
    # on the diagonal of quad 0 both its triangles hold the point, on the vertex (1, 1) six do: the lowest number is taken
    assert owner.tolist() == [0, 0, 0, 2 * 3, 2 * 2, 0]
    val = mo.interpolate(tr, owner, pts[:, 1].copy(), pts[:, 0].copy(), data.reshape(1, -1).astype(np.float64))[0]
    assert val[0] == data[0, 1, 1] and val[1] == (data[0, 0, 0] + data[0, 1, 1]) / 2 and val[2] == (data[0, 0, 0] + data[0, 0, 1]) / 2
    # outside the frame: nothing
    assert mo.mesh_points(flow, np.array([[-0.5, 1.0], [1.0, 2.5], [np.nan, 1.0]]))[1].tolist() == [0, 0, 0]


# ---- the public switch ---------------------------------------------------------------------------------------------------------------
def test_switch_is_off_by_default_and_exported():
    assert ofl.get_mesh_interpolation() is False
    ofl.set_mesh_interpolation()
    try:
        assert ofl.get_mesh_interpolation() is True
    finally:
        ofl.set_mesh_interpolation(False)
    assert ofl.get_mesh_interpolation() is False


def test_with_the_switch_off_every_gate_still_raises(oracle_native):
    f = Flow(torch.ones(2, 5, 7), 's')
    ft = Flow(torch.ones(2, 5, 7), 't')
    ofl.unset_pure_pytorch()
    try:
        for call in (lambda: f.apply(torch.rand(5, 7)),
                     lambda: ofl.apply_flow(torch.ones(2, 5, 7), torch.rand(5, 7), 's'),
                     lambda: ofl.track_pts(torch.ones(2, 5, 7), 't', torch.rand(3, 2)),
                     lambda: ft.track(torch.rand(3, 2)),
                     lambda: f.valid_target(), lambda: ft.valid_source(),
                     lambda: f.combine_with(f * 2, 2), lambda: ft.combine_with(ft * 2, 2), lambda: f.combine_with(f * 2, 1),
                     lambda: f.switch_ref(), lambda: ft.invert()):
            with pytest.raises(NotImplementedError):
                call()
        # one gate stays shut whatever the switch says
        ofl.set_mesh_interpolation()
        with pytest.raises(NotImplementedError):
            ft.combine_with(ft * 2, 2)
    finally:
        ofl.set_mesh_interpolation(False)
        ofl.set_pure_pytorch()


def test_with_pure_pytorch_set_the_switch_changes_nothing(oracle_native, monkeypatch):
    from oflibpytorch_amd import _native

    def boom(*a, **k):
        raise AssertionError("the mesh interpolator ran in PURE_PYTORCH mode")
    monkeypatch.setattr(_native, "mesh_apply", boom, raising=True)
    monkeypatch.setattr(_native, "mesh_points", boom, raising=True)
    g = torch.Generator().manual_seed(3)
    vecs, img, pts = torch.rand(2, 9, 11, generator=g) * 2, torch.rand(3, 9, 11, generator=g), torch.rand(4, 2, generator=g) * 8
    res = []
    for on in (False, True):
        ofl.set_mesh_interpolation(on)
        try:
            res.append((ofl.apply_flow(vecs, img, 's'), ofl.track_pts(vecs, 't', pts), Flow(vecs, 's').apply(img),
                        Flow(vecs, 's').valid_target()))
        finally:
            ofl.set_mesh_interpolation(False)
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_host_plumbing_on_the_oracle(oracle_native, monkeypatch):
    """apply_flow / track_pts / Flow.apply in mesh mode with the kernels replaced by the NumPy oracle: batch broadcast, squeezing,
    dtypes, no grad_fn, the reference's behaviour for integer points."""
    from oflibpytorch_amd import _native

    def mesh_apply(flow, data, *, mask=None, flow_sign=1.0, round_mode=0, want_inside=False, want_owner=False):
        nf, n = flow.shape[0], max(flow.shape[0], data.shape[0])
        u8 = data.dtype == torch.uint8 and round_mode == mo.ROUND_U8
        d = data.detach().numpy() if u8 else data.detach().float().numpy()
        outs = [mo.mesh_apply(flow[b % nf].detach().numpy(), d[b % d.shape[0]], None if mask is None else mask[b % nf].numpy(),
                              flow_sign, round_mode)[0] for b in range(n)]
        return torch.from_numpy(np.stack(outs)), None, None

    def mesh_points(flow, pts, *, mask=None, flow_sign=-1.0):
        res = [mo.mesh_points(flow[b].detach().numpy(), pts[b].detach().numpy(), None, flow_sign) for b in range(flow.shape[0])]
        return torch.from_numpy(np.stack([r[0] for r in res])), torch.from_numpy(np.stack([r[1] for r in res]))
    monkeypatch.setattr(_native, "mesh_apply", mesh_apply)
    monkeypatch.setattr(_native, "mesh_points", mesh_points)
    flow = torch.from_numpy(np.stack([smooth_flow(12, 15, 0), smooth_flow(12, 15, 1)]))
    g = torch.Generator().manual_seed(5)
    img = torch.rand(3, 12, 15, generator=g)
    ofl.unset_pure_pytorch()
    ofl.set_mesh_interpolation()
    try:
        out = ofl.apply_flow(flow, img, 's')                                  # C-H-W target under a batch of two flows
        assert out.shape == (2, 3, 12, 15) and out.dtype == torch.float32
        assert np.array_equal(out[1].numpy(), mo.mesh_apply(flow[1].numpy(), img.numpy())[0])
        assert ofl.apply_flow(flow[0], img[0], 's').shape == (12, 15)
        u8 = (img * 255).to(torch.uint8)
        o8 = ofl.apply_flow(flow[:1], u8, 's')
        assert o8.dtype == torch.uint8 and np.array_equal(o8.numpy(), mo.mesh_apply(flow[0].numpy(), u8.numpy(), round_mode=mo.ROUND_U8)[0])
        i32 = ofl.apply_flow(flow[:1], (img * 1000).to(torch.int32), 's')
        assert i32.dtype == torch.int32
        req = img.clone().requires_grad_(True)
        assert ofl.apply_flow(flow[:1], req, 's').grad_fn is None
        with pytest.raises(ValueError):
            ofl.apply_flow(flow, torch.rand(3, 1, 12, 15), 's')
        # Flow.apply: the valid area is the mask channel thresholded
        warped, valid = Flow(flow[:1], 's').apply(img, return_valid_area=True)
        raw, inside, _ = mo.mesh_apply(flow[0].numpy(), img.numpy())
        assert warped.shape == (3, 12, 15) and np.array_equal(warped.numpy(), raw) and np.array_equal(valid[0].numpy(), inside.astype(bool))
        assert np.array_equal(Flow(flow[:1], 's').valid_target()[0].numpy(), inside.astype(bool))
        # track
        pts = torch.rand(6, 2, generator=g) * 10
        moved = ofl.track_pts(flow, 't', pts)
        assert moved.shape == (2, 6, 2) and moved.dtype == torch.float32
        assert np.array_equal(moved[1].numpy(), mo.track(flow[1].numpy(), pts.numpy()))
        assert ofl.track_pts(flow[:1], 't', pts, int_out=True).dtype == torch.int64
        assert Flow(flow[:1], 't').track(pts).shape == (6, 2)
        with pytest.raises(RuntimeError):                                     # the reference's `+=` of float64 vectors into integer points
            ofl.track_pts(flow[:1], 't', torch.tensor([[2, 3]]))
        p = pts.clone().requires_grad_(True)
        assert ofl.track_pts(flow[:1], 't', p).requires_grad                  # (as the reference: the points pass through `+=`)
    finally:
        ofl.set_mesh_interpolation(False)
        ofl.set_pure_pytorch()


def test_entry_points_reject_bad_arguments_without_a_gpu():
    import ctypes
    from oflibpytorch_amd import _native
    lib = _native.load_library()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)      # never dereferenced: rejected on the argument checks first
    assert lib.ofl_mesh_workspace_ints(1, 1080, 1920, 0) == 16 + 4 * 30 * 68 and lib.ofl_mesh_workspace_ints(2, 16, 16, 1) == 16 + 4 * 2 * 4
    assert lib.ofl_mesh_workspace_ints(1, 1, 8, 0) == -2 and lib.ofl_mesh_workspace_ints(1, 8, 8, 2) == -3
    assert lib.ofl_mesh_plan(null, 0, 1.0, null, 0, 0, one, 1, 8, 8, null) == -1
    assert lib.ofl_mesh_plan(one, 0, 0.5, null, 0, 0, one, 1, 8, 8, null) == -3
    assert lib.ofl_mesh_plan(one, 0, 1.0, null, 0, 0, one, 1, 8, 1, null) == -2
    assert lib.ofl_mesh_apply(one, 0, 1.0, null, 0, null, 0, 0, 0, one, one, 4, one, null, null, 1, 1, 1, 8, 8, null) == -1
    assert lib.ofl_mesh_apply(one, 0, 1.0, null, 0, one, 0, 0, 0, one, one, 4, one, null, null, 2, 3, 1, 8, 8, null) == -2     # nf is 1 or n
    assert lib.ofl_mesh_apply(one, 0, 1.0, null, 0, one, 0, 1, 0, one, one, 4, one, null, null, 1, 1, 1, 8, 8, null) == -3     # uint8 needs ROUND_U8
    assert lib.ofl_mesh_apply(one, 0, 1.0, null, 0, one, 0, 0, 5, one, one, 4, one, null, null, 1, 1, 1, 8, 8, null) == -3
    assert lib.ofl_mesh_points(one, 0, -1.0, null, 0, null, 0, one, one, 4, one, one, 1, 3, 8, 8, null) == -1
    assert lib.ofl_mesh_points(one, 0, -1.0, null, 0, one, 0, one, one, 4, one, one, 1, 0, 8, 8, null) == -2
