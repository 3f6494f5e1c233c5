"""GPU tier of Flow.error_stats / epe_map / epe (ofl_metrics.hip) against tests/flow_error_oracle.py: the map bit for
bit, every count and the maximum exactly, every float64 sum within count * 2^-52 relative of the exact sum (the terms are not negative, so
this bounds ANY summation order), the gradient within 4 float32 ulp of each element of the float64 oracle.

Frames: 2 x 2 and 5 x 7 (h w % 4 != 0: the scalar form), 37 x 53 (h w % 4 != 0, two blocks), 96 x 136 (h w % 4 == 0: 16-byte loads, 13
blocks), 1080 x 1920 (506.25 steps of 1024 pixels for each of the 256 blocks an image gets at most: every block loops 7 or 8 times)."""
import functools
import os

import numpy as np
import pytest
import torch

import flow_error_oracle as feo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [(3, 2, 2), (3, 5, 7), (3, 37, 53), (3, 96, 136)]
LARGE = (2, 1080, 1920)
FRAMES = SMALL + [LARGE]
THRESHOLDS = (1, 3, 5)
GRAD_ULPS = 4.0               # the gradient's bar: float32 ulp of each element's own magnitude
# the tie pixels of the CPU tier: ground truth vectors and the error added to them (e exactly 1, 3, 5, 0, 10, 5; g exactly 0, 10, 40, 5, 50, 100)
TIE_GT = np.array([[0, 0], [6, 8], [24, 32], [3, 4], [30, 40], [60, 80]], np.float32)
TIE_D = np.array([[1, 0], [0, 3], [3, 4], [0, 0], [6, 8], [3, 4]], np.float32)


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _case(n, h, w):
    """(est, gt, est_mask, gt_mask) as NumPy arrays, read-only: a smooth ground truth whose speed runs from 0 to about 60 px across the
    frame, the estimate = ground truth + Gaussian noise of sigma 2.5 per component, both masks with about 20 % holes, the tie pixels
    planted (valid) at the start of every image."""
    rs = np.random.RandomState(1000 * n + 31 * h + w)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    speed = 60.0 * (x / max(w - 1, 1) + y / max(h - 1, 1)) / 2.0
    gt = np.empty((n, 2, h, w), np.float32)
    for i in range(n):
        theta = 2.0 * np.pi * (y / h + 0.37 * i) + 0.5 * np.sin(x / 9.0)
        gt[i, 0], gt[i, 1] = speed * np.cos(theta), speed * np.sin(theta)
    est = gt + (rs.randn(n, 2, h, w) * 2.5).astype(np.float32)
    em, gm = rs.rand(n, h, w) > 0.2, rs.rand(n, h, w) > 0.2
    k = min(len(TIE_GT), h * w)
    for a in (gt, est):
        flat = a.reshape(n, 2, h * w)
        flat[:, :, :k] = (TIE_GT[:k] + (TIE_D[:k] if a is est else 0)).T
    em.reshape(n, -1)[:, :k] = True
    gm.reshape(n, -1)[:, :k] = True
    for a in (est, gt, em, gm):
        a.setflags(write=False)
    return est, gt, em, gm


@functools.lru_cache(maxsize=None)
def _oracle(n, h, w, masked=True):
    est, gt, em, gm = _case(n, h, w)
    return feo.score(est, gt, em if masked else None, gm if masked else None, THRESHOLDS)


@functools.lru_cache(maxsize=None)
def _grad_case(n, h, w):
    """(upstream gradient, the float64 gradient oracle for it)"""
    est, gt, em, gm = _case(n, h, w)
    up = np.array([0.75, -2.0, 1.0], np.float32)[:n]
    scale = (up.astype(np.float64) / _oracle(n, h, w)['count']).astype(np.float32)      # formed as the binding forms it: one rounding
    want = feo.epe_grad(est, gt, em, gm, scale)
    want.setflags(write=False)
    return up, want


def _flows(n, h, w, dtype=torch.float32):
    import oflibpytorch_amd as ofl
    est, gt, em, gm = (torch.from_numpy(a.copy()).to(_dev()) for a in _case(n, h, w))
    return ofl.Flow(est.to(dtype), 't', em), ofl.Flow(gt.to(dtype), 't', gm)


def _records(est, gt, consider_mask=True, want_map=False):
    from oflibpytorch_amd import _native
    return _native.flow_error(est._fv, gt._fv, est._mask if consider_mask else None, gt._mask if consider_mask else None, THRESHOLDS, want_map)


@pytest.mark.parametrize("n,h,w", SMALL[2:] + [LARGE])
def test_the_inputs_show_every_category(n, h, w):
    """A test that cannot see a category is no test of it: on the oracle's own output every threshold count, the Fl count and every
    speed bin lies strictly between 0 and the count, for every image."""
    ref = _oracle(n, h, w)
    for i in range(n):
        c = ref['count'][i]
        assert 0 < c < h * w
        for v in list(ref['n_over'][i]) + [ref['n_fl'][i]] + list(ref['speed_count'][i]):
            assert 0 < v < c, (i, ref['n_over'][i], ref['n_fl'][i], ref['speed_count'][i], c)


@pytest.mark.parametrize("n,h,w", FRAMES)
def test_map_counts_max_and_sums(n, h, w):
    from oflibpytorch_amd import _native
    ref = _oracle(n, h, w)
    est, gt = _flows(n, h, w)
    emap = est.epe_map(gt)
    assert 'flow_error' in _native.last_kernel_name()
    assert emap.dtype == torch.float32 and emap.shape == (n, h, w)
    got = emap.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref['map'].view(np.uint32))               # bit for bit, 0 where not valid
    assert not got[~(_case(n, h, w)[2] & _case(n, h, w)[3])].any()
    rec = _records(est, gt)[0].cpu().numpy()
    assert _native.last_kernel_name().find('flow_error_finish_kernel') >= 0 or _native.last_kernel_name().find('flow_error_kernel') >= 0
    assert rec.shape == (n, 16) and not rec[:, 14:].any() and not rec[:, 3 + len(THRESHOLDS):7].any()
    assert rec[:, 0].tolist() == ref['count'].tolist()
    assert rec[:, 3:6].tolist() == ref['n_over'].tolist() and rec[:, 7].tolist() == ref['n_fl'].tolist()
    assert rec[:, 8:11].tolist() == ref['speed_count'].tolist()
    assert rec[:, 2].tolist() == ref['max'].tolist()
    for i in range(n):
        for got_sum, want, cnt in [(rec[i, 1], ref['sum'][i], ref['count'][i])] + \
                [(rec[i, 11 + b], ref['speed_sum'][i, b], ref['speed_count'][i, b]) for b in range(3)]:
            print("image %d: sum %.17g, exact %.17g, relative difference %.3g, bound %.3g" %
                  (i, got_sum, want, abs(got_sum - want) / max(want, 1e-300), cnt * 2.0 ** -52))
            assert abs(got_sum - want) <= cnt * 2.0 ** -52 * want
    # the API's numbers are torch divisions of the record; epe is the float64 quotient rounded once
    s = est.error_stats(gt, thresholds=THRESHOLDS)
    assert s['count'].tolist() == ref['count'].tolist() and s['speed_count'].tolist() == ref['speed_count'].tolist()
    assert s['max'].tolist() == ref['max'].tolist()
    assert s['epe'].tolist() == (rec[:, 1] / rec[:, 0]).tolist()
    assert s['outliers'].tolist() == (ref['n_over'] / ref['count'][:, None]).tolist() and s['fl'].tolist() == (ref['n_fl'] / ref['count']).tolist()
    assert s['speed_epe'].tolist() == (rec[:, 11:14] / rec[:, 8:11]).tolist()
    assert all(v.device == est.vecs.device for v in s.values())
    e = est.epe(gt)
    assert e.dtype == torch.float32 and e.grad_fn is None
    assert e.tolist() == (rec[:, 1] / rec[:, 0]).astype(np.float32).tolist()


def test_square_roots_are_correctly_rounded_over_the_exponent_range():
    """Components of magnitude 1e-24 .. 1e18 with random mantissas: the sums of squares run from 0 through the denormals to 1e36.  The map
    and the speeds behind the bins must equal np.sqrt on float32 (correctly rounded) bit for bit."""
    import oflibpytorch_amd as ofl
    rs = np.random.RandomState(77)
    n, h, w = 2, 64, 96
    mag = 10.0 ** rs.uniform(-24, 18, (n, 2, h, w))
    d = (mag * rs.uniform(1, 2, (n, 2, h, w)) * rs.choice([-1.0, 1.0], (n, 2, h, w))).astype(np.float32)
    d[1, 1] = d[1, 0] * np.float32(1e-3)                                       # one component dominates
    gt = (10.0 ** rs.uniform(-24, 18, (n, 2, h, w))).astype(np.float32)
    gt[0] = 0                                                                  # image 0: est = d exactly, so du, dv = d
    est = (gt + d).astype(np.float32)
    ref = feo.score(est, gt, None, None, THRESHOLDS)
    sq = (est[:, 0] - gt[:, 0]) ** 2 + (est[:, 1] - gt[:, 1]) ** 2
    assert (sq == 0).any() and ((sq > 0) & (sq < np.finfo(np.float32).tiny)).any() and (sq > 1e30).any() and np.isfinite(sq).all()
    dev = _dev()
    e, g = ofl.Flow(torch.from_numpy(est).to(dev), 't'), ofl.Flow(torch.from_numpy(gt).to(dev), 't')
    assert np.array_equal(e.epe_map(g).cpu().numpy().view(np.uint32), ref['map'].view(np.uint32))
    s = e.error_stats(g, thresholds=THRESHOLDS)
    assert s['speed_count'].tolist() == ref['speed_count'].tolist() and s['max'].tolist() == ref['max'].tolist()
    assert (s['fl'] * h * w).round().tolist() == ref['n_fl'].tolist()
    # the speeds themselves: the map of gt against a zero flow is g
    zero = ofl.Flow(torch.zeros_like(g.vecs), 't')
    assert np.array_equal(zero.epe_map(g).cpu().numpy().view(np.uint32), feo.pixel_terms(est, gt)[3].view(np.uint32))


@pytest.mark.parametrize("n,h,w", FRAMES)
def test_records_do_not_depend_on_the_batch_or_the_run(n, h, w):
    est, gt = _flows(n, h, w)
    rec = _records(est, gt)[0]
    assert torch.equal(_records(est, gt)[0].view(torch.int64), rec.view(torch.int64))                    # a second run
    import oflibpytorch_amd as ofl
    for b in range(n):
        one_e = ofl.Flow(est.vecs[b:b + 1], 't', est.mask[b:b + 1])
        one_g = ofl.Flow(gt.vecs[b:b + 1], 't', gt.mask[b:b + 1])
        assert torch.equal(_records(one_e, one_g)[0].view(torch.int64), rec[b:b + 1].view(torch.int64)), b
        # a copy at another address (the view above starts b images into the batch's storage)
        one_e = ofl.Flow(est.vecs[b:b + 1].clone(), 't', est.mask[b:b + 1].clone())
        assert torch.equal(_records(one_e, one_g)[0].view(torch.int64), rec[b:b + 1].view(torch.int64)), b


@pytest.mark.parametrize("n,h,w", SMALL)
def test_fp16_stored_flows_give_the_bits_of_their_float_copies(n, h, w):
    import oflibpytorch_amd as ofl
    e16, g16 = _flows(n, h, w, torch.float16)
    assert e16._fv.dtype == torch.float16 and g16._fv.dtype == torch.float16
    e32, g32 = ofl.Flow(e16._fv.float(), 't', e16.mask), ofl.Flow(g16._fv.float(), 't', g16.mask)
    want_rec, want_map = _records(e32, g32, want_map=True)
    ref = feo.score(e16._fv.cpu().numpy(), g16._fv.cpu().numpy(), e16.mask.cpu().numpy(), g16.mask.cpu().numpy(), THRESHOLDS)
    assert np.array_equal(want_map.cpu().numpy().view(np.uint32), ref['map'].view(np.uint32))
    for a, b in ((e16, g16), (e16, g32), (e32, g16)):
        rec, emap = _records(a, b, want_map=True)
        assert torch.equal(rec.view(torch.int64), want_rec.view(torch.int64))
        assert torch.equal(emap.view(torch.int32), want_map.view(torch.int32))


@pytest.mark.parametrize("n,h,w", SMALL)
def test_consider_mask_false(n, h, w):
    ref = _oracle(n, h, w, masked=False)
    est, gt = _flows(n, h, w)
    s = est.error_stats(gt, consider_mask=False, thresholds=THRESHOLDS)
    assert s['count'].tolist() == [h * w] * n == ref['count'].tolist()
    assert s['max'].tolist() == ref['max'].tolist() and s['speed_count'].tolist() == ref['speed_count'].tolist()
    assert (s['outliers'] * h * w).round().tolist() == ref['n_over'].tolist() and (s['fl'] * h * w).round().tolist() == ref['n_fl'].tolist()
    np.testing.assert_allclose(s['epe'].cpu().numpy(), ref['sum'] / ref['count'], rtol=h * w * 2.0 ** -52 + 2.0 ** -52, atol=0)
    assert np.array_equal(est.epe_map(gt, consider_mask=False).cpu().numpy().view(np.uint32), ref['map'].view(np.uint32))


def _ulp_check(got, want):
    """within 4 float32 ulp of each element's own magnitude; exact zeros where the oracle has them"""
    got64 = got.astype(np.float64)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    worst = float(np.max(np.abs(got64 - want) / ulp))
    print("worst gradient error: %.3f ulp" % worst)
    assert worst <= GRAD_ULPS
    assert not got[want == 0].any()


@pytest.mark.parametrize("which", ["est", "gt", "both"])
@pytest.mark.parametrize("n,h,w", FRAMES)
def test_gradient(n, h, w, which):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _native
    est_np, gt_np, em_np, gm_np = _case(n, h, w)
    up, want = _grad_case(n, h, w)
    assert (want == 0).any() and (want != 0).any()
    dev = _dev()
    a = torch.from_numpy(est_np.copy()).to(dev).requires_grad_(which in ("est", "both"))
    b = torch.from_numpy(gt_np.copy()).to(dev).requires_grad_(which in ("gt", "both"))
    out = ofl.Flow(a, 't', torch.from_numpy(em_np.copy()).to(dev)).epe(ofl.Flow(b, 't', torch.from_numpy(gm_np.copy()).to(dev)))
    assert type(out.grad_fn).__name__.startswith("EpeFn")
    out.backward(torch.from_numpy(up).to(dev))
    assert 'flow_epe_grad_kernel' in _native.last_kernel_name()
    if a.requires_grad:
        _ulp_check(a.grad.cpu().numpy(), want)
    else:
        assert a.grad is None
    if b.requires_grad:
        _ulp_check(b.grad.cpu().numpy(), -want)
    else:
        assert b.grad is None
    if which == "both":
        assert torch.equal(b.grad.view(torch.int32), (-a.grad).view(torch.int32))
        assert torch.equal((a.grad == 0), (b.grad == 0))


def test_an_image_without_valid_pixels():
    import math
    import oflibpytorch_amd as ofl
    n, h, w = SMALL[3]
    est, gt = _flows(n, h, w)
    rec = _records(est, gt)[0]
    m = est.mask.clone()
    m[1] = False
    v = est.vecs.clone().requires_grad_()
    blind = ofl.Flow(v, 't', m)
    s = blind.error_stats(gt)
    assert s['count'].tolist()[1] == 0 and math.isnan(s['epe'][1]) and s['max'][1] == 0 and not s['speed_count'][1].any()
    assert not blind.epe_map(gt)[1].any()
    got = _records(blind, gt)[0]
    assert not got[1].any()
    assert torch.equal(got[[0, 2]].view(torch.int64), rec[[0, 2]].view(torch.int64))                    # the neighbours: untouched
    e = blind.epe(gt)
    assert math.isnan(e[1].item()) and torch.isfinite(e[[0, 2]]).all()
    e.backward(torch.ones(n, device=e.device))
    assert not v.grad[1].any() and v.grad[0].any() and v.grad[2].any() and torch.isfinite(v.grad).all()


def test_kitti_fixture_against_itself_shifted():
    import oflibpytorch_amd as ofl
    gt = ofl.Flow.from_kitti(os.path.join(ROOT, 'tests', 'golden', 'loaders', 'kitti.png'), device='cuda')
    assert gt.mask.any() and not gt.mask.all()
    shift = torch.tensor([3.0, 4.0], device=gt.vecs.device).reshape(1, 2, 1, 1)
    est = ofl.Flow(gt.vecs + shift, 's', gt.mask)             # multiples of 1 / 64 below 2^9: the sums are exact
    s = est.error_stats(gt)
    assert s['count'].tolist() == [int(gt.mask.sum())]
    assert s['epe'].tolist() == [5.0] and s['max'].tolist() == [5.0] and est.epe(gt).tolist() == [5.0]
    assert s['outliers'][:, 1].tolist() == [1.0] and s['outliers'][:, 0].tolist() == [1.0] and s['outliers'][:, 2].tolist() == [0.0]
    emap = est.epe_map(gt)
    assert (emap[gt.mask] == 5).all() and not emap[~gt.mask].any()
