"""GPU tier of the triangle-mesh interpolator (ofl_mesh.hip) against the NumPy oracle tests/mesh_oracle.py: the triangle
each pixel took and the inside byte EXACT, the values BIT-EQUAL after the rounding to float32 (the kernel keeps the oracle's operation
order, no tolerance) -- over the host tier's cases, every frame size around the 64 x 16 tile, batch broadcast both ways, C = 1 / 3 / 8,
uint8 and integer targets, masks with holes, a fold, a stretch that lays one triangle over many tiles, the public API, run-to-run and
batch determinism, and one 1080p frame."""
import numpy as np
import pytest
import torch

import mesh_oracle as mo
import oflibpytorch_amd as ofl
from oflibpytorch_amd import Flow, _native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@pytest.fixture
def mesh_mode():
    ofl.unset_pure_pytorch()
    ofl.set_mesh_interpolation()
    yield
    ofl.set_mesh_interpolation(False)
    ofl.set_pure_pytorch()


def _smooth(n, h, w, scale, seed):
    g = torch.Generator().manual_seed(seed)
    lo = torch.randn(n, 2, 5, 7, generator=g) * scale
    return torch.nn.functional.interpolate(lo, size=(h, w), mode='bicubic', align_corners=True).contiguous()


def _data(n, c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, c, h, w, generator=g) * 255


def _holes(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(n, h, w, generator=g) > 0.1
    m[:, h // 4: h // 2, w // 3: w // 2] = False
    return m


def _check_apply(flow, data, dev, mask=None, sign=1.0, round_mode=0):
    """kernels vs oracle for every image of the (broadcast) batch: owner, inside, values -- all exact"""
    out, inside, owner = _native.mesh_apply(flow.to(dev), data.to(dev), mask=None if mask is None else mask.to(dev), flow_sign=sign,
                                            round_mode=round_mode, want_inside=True, want_owner=True)
    n = max(flow.shape[0], data.shape[0])
    assert out.shape == (n,) + tuple(data.shape[1:]) and inside.shape == owner.shape == (n,) + tuple(data.shape[2:])
    u8 = data.dtype == torch.uint8 and round_mode == mo.ROUND_U8
    d = data.numpy() if u8 else data.float().numpy()
    for b in range(n):
        fb, db = flow[b % flow.shape[0]].numpy(), d[b % d.shape[0]]
        want, w_inside, w_owner = mo.mesh_apply(fb, db, None if mask is None else mask[b % mask.shape[0]].numpy(), sign, round_mode)
        assert np.array_equal(owner[b].cpu().numpy(), w_owner), "owner, image %d" % b
        assert np.array_equal(inside[b].cpu().numpy(), w_inside), "inside, image %d" % b
        got = out[b].cpu().numpy()
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8)), "values, image %d" % b
    return out, inside, owner


@pytest.mark.parametrize("size", [(40, 56), (33, 47), (25, 61)])
@pytest.mark.parametrize("c", [1, 3])
def test_host_cases_smooth(dev, size, c):
    from test_mesh_host import smooth_flow
    h, w = size
    for seed in range(3):
        flow = torch.from_numpy(smooth_flow(h, w, seed))[None]
        _check_apply(flow, _data(1, c, h, w, seed) / 255, dev)
        _check_apply(flow, _data(1, c, h, w, seed).to(torch.uint8), dev, round_mode=mo.ROUND_U8)


def test_host_cases_hand_built(dev):
    # identity (every quad a tie), the other diagonal, a masked vertex, a non-finite vertex, a fold, degenerate quads
    z = torch.zeros(1, 2, 6, 7)
    out, inside, owner = _check_apply(z, _data(1, 2, 6, 7, 0), dev)
    assert bool(inside.all()) and torch.equal(out.cpu(), _data(1, 2, 6, 7, 0))
    f = torch.zeros(1, 2, 2, 2)
    f[0, :, 1, 0] = torch.tensor([0.25, -0.25])
    _check_apply(f, _data(1, 1, 2, 2, 1), dev)
    f = torch.full((1, 2, 6, 6), 0.25)
    m = torch.ones(1, 6, 6, dtype=torch.bool)
    m[0, 3, 2] = False
    _, inside, _ = _check_apply(f, _data(1, 1, 6, 6, 2), dev, mask=m)
    assert inside[0, 3, 3] == 0 and inside[0, 2, 2] == 1
    bad = f.clone()
    bad[0, 0, 3, 2] = float('inf')
    _check_apply(bad, _data(1, 1, 6, 6, 2), dev)               # (the C ABI drops the vertex; the public API rejects the flow)
    fold = torch.zeros(1, 2, 4, 8)
    fold[0, 0, :, 4:] = -3.0
    _, _, owner = _check_apply(fold, _data(1, 1, 4, 8, 3), dev)
    assert owner[0, 1, 2] == 2 * 1 and owner[0, 2, 3] == 2 * (7 + 2)
    flat = torch.zeros(1, 2, 3, 3)
    flat[0, 0, :, 1] = 1.0
    _check_apply(flat, _data(1, 1, 3, 3, 4), dev)


@pytest.mark.parametrize("h", [2, 15, 16, 17, 31, 32, 33])
@pytest.mark.parametrize("w", [2, 63, 64, 65, 127, 128, 129])
def test_tile_boundaries(dev, h, w):
    flow = _smooth(1, h, w, 2.0, h * 1000 + w)
    _check_apply(flow, _data(1, 2, h, w, 7), dev)


@pytest.mark.parametrize("c", [1, 3, 8])
def test_batch_broadcast_channels_and_sign(dev, c):
    h, w = 37, 70
    flow3, data3 = _smooth(3, h, w, 3.0, 11), _data(3, c, h, w, 12)
    _check_apply(flow3, data3, dev)
    _check_apply(flow3[:1], data3, dev)                       # one flow, three targets
    _check_apply(flow3, data3[:1], dev)                       # three flows, one target
    _check_apply(flow3[:1], data3[:1], dev, sign=-1.0)


def test_integer_targets_and_masks_with_holes(dev):
    h, w = 45, 83
    flow, mask = _smooth(2, h, w, 3.0, 21), _holes(2, h, w, 22)
    _check_apply(flow, _data(2, 3, h, w, 23).to(torch.uint8), dev, mask=mask, round_mode=mo.ROUND_U8)
    _check_apply(flow, _data(2, 3, h, w, 23) - 100, dev, mask=mask, round_mode=mo.ROUND_U8)      # fp32 in, rounded and clamped
    _check_apply(flow, (_data(2, 1, h, w, 24) * 40 - 3000).round(), dev, mask=mask, round_mode=mo.ROUND_RINT)
    _check_apply(flow[:1], _data(2, 1, h, w, 25), dev, mask=mask[:1])


def test_fold_and_rough_flow(dev):
    h, w = 50, 90
    g = torch.Generator().manual_seed(31)
    rough = _smooth(1, h, w, 2.0, 32) + torch.randn(1, 2, h, w, generator=g) * 1.5             # folds everywhere
    _check_apply(rough, _data(1, 2, h, w, 33), dev)


def test_stretch_one_triangle_over_many_tiles(dev):
    h, w = 48, 200
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    # scaling by 40 about (3, 2): the quads next to the centre cover 40 x 40 pixels each -- several 64 x 16 tiles
    flow = torch.stack([(xx - 3) * 39, (yy - 2) * 39])[None] + _smooth(1, h, w, 0.3, 41)
    out, inside, owner = _check_apply(flow, _data(1, 3, h, w, 42), dev)
    assert len(torch.unique(owner[owner >= 0])) < 60 and float(inside.float().mean()) > 0.9


def test_points_against_the_oracle(dev):
    h, w = 41, 77
    flow = _smooth(2, h, w, 3.0, 51)
    g = torch.Generator().manual_seed(52)
    pts = torch.rand(2, 500, 2, generator=g) * torch.tensor([h + 4.0, w + 4.0]) - 2.0            # some outside the frame
    pts[:, :40] = pts[:, :40].round()
    pts[0, 40] = float('nan')
    for p in (pts, pts[:1]):
        vecs, inside = _native.mesh_points(flow.to(dev), p.to(dev))
        for b in range(2):
            wv, wi = mo.mesh_points(flow[b].numpy(), p[b % p.shape[0]].numpy())
            assert np.array_equal(inside[b].cpu().numpy(), wi)
            assert np.array_equal(vecs[b].cpu().numpy().view(np.uint64), wv.view(np.uint64))
    assert 0 < int(inside.sum()) < inside.numel()
    fold = torch.zeros(1, 2, 4, 8)
    fold[0, 0, :, 4:] = 3.0                                    # 't': start points grid - flow fold back
    q = torch.tensor([[[1.5, 2.25], [0.0, 0.0], [3.0, 4.0], [2.0, 1.0]]])
    vecs, inside = _native.mesh_points(fold.to(dev), q.to(dev))
    wv, wi = mo.mesh_points(fold[0].numpy(), q[0].numpy())
    assert np.array_equal(inside[0].cpu().numpy(), wi) and np.array_equal(vecs[0].cpu().numpy(), wv)


def test_public_api(dev, mesh_mode):
    h, w = 38, 66
    flow, img = _smooth(2, h, w, 2.5, 61), _data(1, 3, h, w, 62)[0]
    want = [mo.mesh_apply(flow[b].numpy(), img.numpy()) for b in range(2)]
    out = ofl.apply_flow(flow.to(dev), img.to(dev), 's')
    assert out.shape == (2, 3, h, w) and out.dtype == torch.float32 and out.grad_fn is None
    assert all(np.array_equal(out[b].cpu().numpy(), want[b][0]) for b in range(2))
    assert ofl.apply_flow(flow[0].to(dev), img[0].to(dev), 's').shape == (h, w)
    mask = _holes(2, h, w, 63)
    o8 = ofl.apply_flow(flow.to(dev), img.to(torch.uint8).to(dev), 's', mask.to(dev))
    w8 = mo.mesh_apply(flow[1].numpy(), img.to(torch.uint8).numpy(), mask[1].numpy(), round_mode=mo.ROUND_U8)[0]
    assert o8.dtype == torch.uint8 and np.array_equal(o8[1].cpu().numpy(), w8)
    oi = ofl.apply_flow(flow[:1].to(dev), (img * 10).to(torch.int32).to(dev), 's')
    wi = mo.mesh_apply(flow[0].numpy(), (img * 10).to(torch.int32).float().numpy(), round_mode=mo.ROUND_RINT)[0]
    assert oi.dtype == torch.int32 and np.array_equal(oi.cpu().numpy(), wi.astype(np.int32))
    with pytest.raises(ValueError):
        ofl.apply_flow(torch.full((2, h, w), float('nan')).to(dev), img.to(dev), 's')            # non-finite flow: rejected as today
    with pytest.raises(ValueError):
        ofl.track_pts(torch.full((2, h, w), float('inf')).to(dev), 't', torch.rand(3, 2))
    req = img.clone().to(dev).requires_grad_(True)
    assert ofl.apply_flow(flow[:1].to(dev), req, 's').grad_fn is None
    # Flow.apply: the warped tensor, and the valid area = the mask channel at 0.99999
    fl = Flow(flow[:1], 's', device=dev)
    warped, valid = fl.apply(img.to(dev), return_valid_area=True)
    assert np.array_equal(warped.cpu().numpy(), want[0][0]) and np.array_equal(valid[0].cpu().numpy(), want[0][1].astype(bool))
    assert fl.apply(img.to(torch.uint8).to(dev)).dtype == torch.uint8
    assert np.array_equal(fl.valid_target()[0].cpu().numpy(), want[0][1].astype(bool))
    fm = Flow(flow[:1], 's', mask[:1], device=dev)
    wm = mo.mesh_apply(flow[0].numpy(), torch.cat((img, mask[:1].float())).numpy(), mask[0].numpy())[0]
    warped, valid = fm.apply(img.to(dev), return_valid_area=True)
    assert np.array_equal(warped.cpu().numpy(), wm[:3]) and np.array_equal(valid[0].cpu().numpy(), wm[3] > 0.99999)
    # a Flow as the target, and what is built on apply: switch_ref, invert, combine_with modes 1 - 3 run and give a flow
    other = Flow(_smooth(1, h, w, 1.0, 64), 's', device=dev)
    res = fl.apply(other)
    wf = mo.mesh_apply(flow[0].numpy(), torch.cat((other.vecs[0].cpu(), torch.ones(1, h, w))).numpy())[0]
    assert res.ref == 's' and np.array_equal(res.vecs[0].cpu().numpy(), wf[:2]) and np.array_equal(res.mask[0].cpu().numpy(), wf[2] > 0.99999)
    for made in (fl.switch_ref(), fl.invert(), fl.combine_with(other, 1), fl.combine_with(other, 2), fl.combine_with(other, 3)):
        assert isinstance(made, Flow) and made.shape == (1, h, w) and bool(torch.isfinite(made.vecs).all())
    assert np.array_equal(fl.combine_with(other, 2).vecs.cpu().numpy(), fl.apply(other - fl).vecs.cpu().numpy())     # :1768
    # padding goes through the replicated pad and the same interpolator
    big = _data(1, 2, h + 5, w + 7, 65)[0]
    pm = torch.nn.functional.pad(torch.ones(h, w, dtype=torch.bool), (3, 4, 2, 3))                # (the padded flow's mask: False in the pad)
    wp = mo.mesh_apply(torch.nn.functional.pad(flow[:1], (3, 4, 2, 3), mode='replicate')[0].numpy(), big.numpy(), pm.numpy())[0]
    assert np.array_equal(fl.apply(big.to(dev), padding=[2, 3, 3, 4], cut=False).cpu().numpy(), wp)
    # track
    g = torch.Generator().manual_seed(66)
    pts = torch.rand(50, 2, generator=g) * torch.tensor([h - 1.0, w - 1.0])
    moved = ofl.track_pts(flow.to(dev), 't', pts.to(dev))
    assert moved.shape == (2, 50, 2) and moved.dtype == torch.float32
    assert all(np.array_equal(moved[b].cpu().numpy(), mo.track(flow[b].numpy(), pts.numpy())) for b in range(2))
    ft = Flow(flow[:1], 't', device=dev)
    assert np.array_equal(ft.track(pts.to(dev)).cpu().numpy(), mo.track(flow[0].numpy(), pts.numpy()))
    assert ft.track(pts.to(dev), int_out=True).dtype == torch.int64
    assert np.array_equal(ft.valid_source()[0].cpu().numpy(), mo.mesh_apply(flow[0].numpy(), np.ones((1, h, w), np.float32), sign=-1.0)[0][0] == 1)
    with pytest.raises(RuntimeError):
        ofl.track_pts(flow[:1].to(dev), 't', torch.tensor([[2, 3]]))
    with pytest.raises(NotImplementedError):
        ft.combine_with(ft * 2, 2)                                                               # the one gate kept


def test_pure_pytorch_mode_is_untouched_by_the_switch(dev):
    h, w = 30, 50
    flow, img = _smooth(1, h, w, 2.0, 71).to(dev), _data(1, 3, h, w, 72).to(dev)
    a = ofl.apply_flow(flow, img, 's')
    ofl.set_mesh_interpolation()
    try:
        b = ofl.apply_flow(flow, img, 's')
        assert _native.last_kernel_name().find('mesh') < 0
    finally:
        ofl.set_mesh_interpolation(False)
    assert torch.equal(a, b)


def test_determinism(dev):
    h, w = 70, 150
    g = torch.Generator().manual_seed(81)
    flow = (_smooth(4, h, w, 3.0, 82) + torch.randn(4, 2, h, w, generator=g) * 0.8).to(dev)
    data, mask = _data(4, 3, h, w, 83).to(dev), _holes(4, h, w, 84).to(dev)
    a = _native.mesh_apply(flow, data, mask=mask, want_inside=True, want_owner=True)
    b = _native.mesh_apply(flow, data, mask=mask, want_inside=True, want_owner=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for i in range(4):
        alone = _native.mesh_apply(flow[i:i + 1], data[i:i + 1], mask=mask[i:i + 1], want_inside=True, want_owner=True)
        assert all(torch.equal(x[i:i + 1], y) for x, y in zip(a, alone))
    pts = (torch.rand(4, 300, 2, generator=g) * torch.tensor([h - 1.0, w - 1.0])).to(dev)
    p1, p2 = _native.mesh_points(flow, pts), _native.mesh_points(flow, pts)
    assert torch.equal(p1[0], p2[0]) and torch.equal(p1[1], p2[1])
    assert torch.equal(_native.mesh_points(flow[2:3], pts[2:3])[0], p1[0][2:3])


def test_one_1080p_frame(dev):
    h, w = 1080, 1920
    flow = _smooth(1, h, w, 8.0, 91)
    _check_apply(flow, _data(1, 3, h, w, 92), dev)
