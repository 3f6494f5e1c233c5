"""GPU tier of Flow.visualise_arrows / visualise_flow_arrows (ofl_arrows.hip): BIT-EXACT against the NumPy oracle
(tests/arrows_oracle.py), no tolerance: the reference's test scale over every argument, smooth random flows at odd sizes and on
the smallest frames, dense grids, arrows that span or leave the frame, the far-end-point rule, degenerate percentiles, fp16
storage, the API's forms, batch (in)dependence, run-to-run identity and one 1080p batch."""
import itertools

import numpy as np
import pytest
import torch

import arrows_oracle as ao

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _smooth(n, h, w, scale, seed, dev):
    g = torch.Generator().manual_seed(seed)
    lo = torch.randn(n, 2, 5, 7, generator=g) * scale
    f = torch.nn.functional.interpolate(lo, size=(h, w), mode='bicubic', align_corners=True)
    f[:, :, : h // 7, : w // 9] = 0                         # a patch of zero vectors
    return f.contiguous().to(dev)


def _mask(n, h, w, seed, dev):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(n, h, w, generator=g) > 0.2
    m[:, h // 4: h // 2, w // 3: w // 2] = False
    return m.to(dev)


def _background(h, w, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (h, w, 3)).astype(np.uint8)


def _img_forms(bg, n):
    """{name: (the argument, the oracle's N-H-W-3 view of it)}: every form the method accepts"""
    np1, np_n = bg[None], np.stack([np.roll(bg, 3 * i, axis=1) for i in range(n)])
    pt = torch.from_numpy(bg).permute(2, 0, 1)
    return {'none': (None, None), 'np': (bg, bg), 'np_1': (np1, np1), 'np_n': (np_n, np_n), 'pt': (pt, bg),
            'pt_1': (pt.unsqueeze(0), np1), 'pt_n_expand': (pt.unsqueeze(0).expand(n, -1, -1, -1), np1),
            'pt_n': (torch.from_numpy(np_n).permute(0, 3, 1, 2), np_n)}


def _check(fl, flow, mask, ref, img=None, img_np=None, **kw):
    exp = ao.visualise_arrows(flow.cpu().float().numpy(), ref, None if mask is None else mask.cpu().numpy(), img=img_np, **kw)
    got = fl.visualise_arrows(img=img, return_tensor=False, **kw)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == exp.shape
    if not np.array_equal(got, exp):
        bad = np.argwhere((got != exp).any(-1))
        raise AssertionError("%d pixels differ, first (image, row, column) %s: got %s, expected %s -- %s"
                             % (len(bad), bad[0], got[tuple(bad[0])], exp[tuple(bad[0])], kw))
    return exp


def _reference_scale_flows(ref, dev):
    """The flows of the reference's test (test_flow_class.py:1795-1803) at its scale: three flows from transforms, batched,
    a rectangular mask"""
    import oflibpytorch_amd as ofl
    h, w = 128, 160
    mask = np.zeros((h, w))
    mask[50:-50, 20:-20] = 1
    flow1 = ofl.batch_flows((ofl.Flow.from_transforms([['translation', 10, -8]], (h, w), ref, mask, device=dev),
                             ofl.Flow.from_transforms([['translation', -5, 10]], (h, w), ref, mask, device=dev),
                             ofl.Flow.from_transforms([['rotation', 30, 50, 30]], (h, w), ref, mask, device=dev)))
    flow2 = ofl.Flow.from_transforms([['rotation', 10, 30, 20]], (h, w), ref, mask, device=dev)
    return flow1, flow2


@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("scaling", [None, 0.1, 1, 2])
def test_reference_scale_all_arguments(ref, scaling, dev):
    flow1, flow2 = _reference_scale_flows(ref, dev)
    bg = _background(128, 160, 5)
    for fl in (flow1, flow2):
        forms = _img_forms(bg, fl.shape[0])
        # every image form once per (show_mask, borders); colour and thickness cycle through their values alongside
        cyc = itertools.cycle(itertools.product((None, (100, 100, 100), (10, 200, 30)), (1, 2, 6)))
        for show_mask, borders in itertools.product((False, True), (False, True)):
            for name, (arg, as_np) in forms.items():
                if fl.shape[0] == 1 and name in ('np_n', 'pt_n', 'pt_n_expand'):
                    continue
                colour, thickness = next(cyc)
                _check(fl, fl.vecs, fl.mask, ref, img=arg, img_np=as_np, grid_dist=10, scaling=scaling, show_mask=show_mask,
                       show_mask_borders=borders, colour=colour, thickness=thickness)
    # and the full product of colour x thickness on one image form
    for colour, thickness in itertools.product((None, (100, 100, 100)), (1, 2, 6)):
        _check(flow1, flow1.vecs, flow1.mask, ref, img=bg, img_np=bg, grid_dist=10, scaling=scaling, show_mask=True,
               show_mask_borders=True, colour=colour, thickness=thickness)


@pytest.mark.parametrize("shape", [(3, 37, 53), (2, 40, 64), (1, 2, 2), (2, 2, 3), (1, 3, 2), (2, 4, 5), (1, 5, 7)])
@pytest.mark.parametrize("ref", ['s', 't'])
def test_smooth_flows_odd_sizes_and_smallest_frames(shape, ref, dev):
    import oflibpytorch_amd as ofl
    n, h, w = shape
    flow = _smooth(n, h, w, 5.0, 3 + h, dev)
    mask = _mask(n, h, w, 4 + w, dev)
    fl = ofl.Flow(flow, ref, mask)
    bg = np.stack([_background(h, w, 7 + i) for i in range(n)])
    for grid_dist in (None, 1, 2, 5, 10):
        if grid_dist is not None and grid_dist > min(h, w) // 2 and grid_dist != 10:
            continue                                            # (10 stays: it exercises the reset on small frames)
        for scaling, thickness, show in ((None, 1, False), (1, 2, True), (2.5, 6, True), (0.1, 3, False)):
            _check(fl, flow, mask, ref, img=bg, img_np=bg, grid_dist=grid_dist, scaling=scaling, thickness=thickness,
                   show_mask=show, show_mask_borders=show)
    _check(ofl.Flow(flow, ref), flow, None, ref, show_mask=True, show_mask_borders=True)      # no mask: all True


@pytest.mark.parametrize("ref", ['s', 't'])
def test_dense_grids_and_frame_spanning_arrows(ref, dev):
    import oflibpytorch_amd as ofl
    n, h, w = 2, 70, 150
    flow = _smooth(n, h, w, 3.0, 71, dev)
    mask = _mask(n, h, w, 72, dev)
    fl = ofl.Flow(flow, ref, mask)
    for grid_dist in (1, 2):                                    # every (second) pixel a grid point: long lists
        for scaling, thickness in ((None, 1), (1, 2), (4, 3)):
            _check(fl, flow, mask, ref, grid_dist=grid_dist, scaling=scaling, thickness=thickness)
    for grid_dist, scaling, thickness in ((10, 40, 1), (10, 40, 6), (7, 300, 2), (3, 60, 1)):   # arrows across and out of the frame
        _check(fl, flow, mask, ref, grid_dist=grid_dist, scaling=scaling, thickness=thickness, show_mask=True)


@pytest.mark.parametrize("ref", ['s', 't'])
def test_far_end_points_zero_flow_and_zero_percentile(ref, dev):
    import oflibpytorch_amd as ofl
    n, h, w = 2, 40, 60
    flow = _smooth(n, h, w, 2.0, 81, dev)
    fl = ofl.Flow(flow, ref)
    # scaled magnitudes on both sides of 2^20: some arrows skipped by the rule, the others far out of the frame
    mag = float(torch.linalg.vector_norm(flow[:, :, 5::10, 5::10], dim=1).median())
    _check(fl, flow, None, ref, grid_dist=10, scaling=2.0 ** 20 / mag)
    _check(fl, flow, None, ref, grid_dist=10, scaling=1e30)
    zero = torch.zeros(n, 2, h, w, device=dev)
    exp = _check(ofl.Flow(zero, ref), zero, None, ref, grid_dist=10)                 # red pixels only
    pts = ao.grid_points(h, w, 10)
    assert np.all(exp[:, pts[:, 0], pts[:, 1]] == [0, 0, 255]) and int((exp != 255).any(-1).sum()) == n * len(pts)
    one = zero.clone()
    one[1, :, 15, 25] = torch.tensor([3.0, -2.0], device=dev)      # 1200 grid points, one moves: the percentile is 0, scaling inf
    pts = ao.grid_points(h, w, 2)
    assert ao.default_scaling(ao.sample(one.cpu().numpy(), 2)[2], 2) == np.inf
    exp = _check(ofl.Flow(one, ref), one, None, ref, grid_dist=2)
    assert int((exp != 255).any(-1).sum()) == n * len(pts)        # the moving point's arrow is skipped: red pixels only
    _check(ofl.Flow(one, ref), one, None, ref, grid_dist=2, scaling=3)


def test_fp16_stored_flow(dev):
    import oflibpytorch_amd as ofl
    for (n, h, w) in ((2, 37, 53), (3, 48, 64)):
        f16 = _smooth(n, h, w, 6.0, 31 + w, dev).half()
        mask = _mask(n, h, w, 32, dev)
        for ref in ('s', 't'):
            fl = ofl.Flow(f16, ref, mask)
            assert fl._half is not None                       # (read as fp16 planes by the kernels)
            for scaling in (None, 1.5):
                _check(fl, f16.float(), mask, ref, grid_dist=6, scaling=scaling, thickness=2, show_mask=True, show_mask_borders=True)
            assert fl._half is not None


def test_api_forms_and_caller_image_unchanged(dev):
    import oflibpytorch_amd as ofl
    n, h, w = 3, 45, 70
    flow = _smooth(n, h, w, 4.0, 91, dev)
    mask = _mask(n, h, w, 92, dev)
    fl = ofl.Flow(flow, 't', mask)
    bg = np.stack([_background(h, w, 93 + i) for i in range(n)])
    for arg in (bg, torch.from_numpy(bg).permute(0, 3, 1, 2).contiguous(), torch.from_numpy(bg).permute(0, 3, 1, 2).to(dev)):
        keep = arg.copy() if isinstance(arg, np.ndarray) else arg.clone()
        t = fl.visualise_arrows(10, arg, 2, True, True, None, 2)
        a = fl.visualise_arrows(10, arg, 2, True, True, None, 2, return_tensor=False)
        assert isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.uint8 and t.shape == (n, 3, h, w)
        assert isinstance(a, np.ndarray) and a.shape == (n, h, w, 3)
        assert np.array_equal(np.moveaxis(t.cpu().numpy(), 1, -1), a)
        assert np.array_equal(a, ao.visualise_arrows(flow.cpu().numpy(), 't', mask.cpu().numpy(), 10, bg, 2, True, True, None, 2))
        assert (np.array_equal(arg, keep) if isinstance(arg, np.ndarray) else torch.equal(arg, keep))     # never written to
    for ref in ('s', 't'):
        m = ofl.Flow(flow, ref).visualise_arrows(10, bg, 1.5, thickness=3)
        f = ofl.visualise_flow_arrows(flow, ref, 10, bg, 1.5, thickness=3)
        assert torch.equal(m, f)
        f3 = ofl.visualise_flow_arrows(flow[0], ref, 10, bg[0], 1.5, thickness=3)
        assert f3.shape == (3, h, w) and torch.equal(f3, m[0])
        a3 = ofl.visualise_flow_arrows(flow[0].cpu().numpy(), ref, 10, None, 1.5, return_tensor=False)
        assert isinstance(a3, np.ndarray) and a3.shape == (h, w, 3)
    cpu = ofl.Flow(flow.cpu(), 't', mask.cpu()).visualise_arrows(10, bg, 2)
    assert cpu.device.type == 'cpu' and torch.equal(cpu, fl.visualise_arrows(10, bg, 2).cpu())


def test_batch_independence_and_batch_wide_scaling(dev):
    import oflibpytorch_amd as ofl
    n, h, w = 16, 45, 70
    flow = _smooth(n, h, w, 8.0, 51, dev) * torch.linspace(0.1, 3, n, device=dev).view(n, 1, 1, 1)
    mask = _mask(n, h, w, 52, dev)
    fl = ofl.Flow(flow, 't', mask)
    args = dict(grid_dist=8, show_mask=True, show_mask_borders=True, thickness=2)
    a = fl.visualise_arrows(scaling=1.3, **args)
    assert torch.equal(a, fl.visualise_arrows(scaling=1.3, **args))                   # run to run
    singles = torch.cat([ofl.Flow(flow[i:i + 1], 't', mask[i:i + 1]).visualise_arrows(scaling=1.3, **args) for i in range(n)])
    assert torch.equal(a, singles)                                                    # a given scaling: images independent
    d = fl.visualise_arrows(**args)
    assert torch.equal(d, fl.visualise_arrows(**args))
    _, pts, mags, _ = ao.sample(flow.cpu().numpy(), 8)
    s = ao.default_scaling(mags, 8)                                                  # ONE scalar for the batch
    assert s.dtype == np.float32
    assert torch.equal(d, fl.visualise_arrows(scaling=float(s), **args))
    alone = ofl.Flow(flow[:1], 't', mask[:1]).visualise_arrows(**args)
    assert not torch.equal(alone, d[:1])                                              # (the percentile of image 0 alone differs)
    from oflibpytorch_amd import _native
    assert np.float32(_native.arrows_scale(flow, 8).item()).view(np.uint32) == s.view(np.uint32)


def test_full_hd_batch_of_four(dev):
    import oflibpytorch_amd as ofl
    n, h, w = 4, 1080, 1920
    flow = _smooth(n, h, w, 12.0, 21, dev)
    mask = _mask(n, h, w, 22, dev)
    bg = _background(h, w, 23)
    for ref in ('s', 't'):
        fl = ofl.Flow(flow, ref, mask)
        _check(fl, flow, mask, ref, img=bg, img_np=bg, grid_dist=20, show_mask=True, show_mask_borders=True, thickness=2)
    _check(ofl.Flow(flow, 't', mask), flow, mask, 't', grid_dist=20)
