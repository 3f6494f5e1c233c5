"""GPU tier of tests/loss_specials.py: the fused loss and metric kernels (ofl_photometric.hip, ofl_census.hip, ofl_consistency.hip,
ofl_smoothness.hip, ofl_metrics.hip) at named sample positions and on NaN, +-inf and +-FLT_MAX, against the oracles of their own tiers
(the bars are those of tests/test_gpu_<family>.py, taken class by class):

  forward    maps, masks and per-pixel outputs equal the oracle on the terms of special_values.same_bits (equal bits where finite, NaN
             where NaN, the same infinity) wherever the family's own test demands bits; where it allows ulps (the smoothness weight,
             the census pow) the class is equal and the finite values are within those ulps; unknown pixels are exactly +0
  records    counts exact; a sum is NaN if a term is, else +inf if a term is, else within the family's bound of math.fsum; the maximum
             is the largest term that is not NaN; the loss is the quotient of the call's own record; the clean image of a batch (image
             3) keeps the bits it has in the finite variant
  isolation  a pixel none of whose taps (stencil, patch) holds a planted element carries the bits of the finite variant, map and
             gradient; the set is computed from the taps, not from the outputs
  gradient   exactly +0 where the pixel is not known (a vector of its own that is not finite included); the oracle's class where its
             value or A is not finite; within 2^-22 A + ulp32(want) elsewhere (error_stats: 4 ulp)

tests/test_loss_specials_host.py shows on the CPU that no case is empty of any of this."""
import numpy as np
import pytest
import torch

import census_oracle as cen
import consistency_oracle as co
import flow_error_oracle as feo
import loss_specials as ls
import photometric_oracle as po
import smoothness_oracle as so
import special_values as sv

gpu = pytest.mark.gpu
EPS = 1e-3
N = ls.N
CONS_ALPHA, CONS_BETA = 1.0, 0.5


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _t(x, grad=False):
    t = torch.from_numpy(np.array(x)).to(_dev())
    return t.requires_grad_(True) if grad else t


def _np(t):
    return t.detach().cpu().numpy()


def _same(got, want, what):
    assert sv.same_bits(got, want).all(), (what, sv.describe(got, want))


def _same64(got, want, what):
    """float64 record fields that are exact: equal, the same infinity; a NaN is expected nowhere"""
    assert not np.isnan(want).any() and np.array_equal(got, want), (what, got, want)


def _up():
    return torch.tensor(ls.UPSTREAM, device=_dev())


def _wrapped(v, ref, mask):
    import oflibpytorch_amd as ofl
    return ofl.Flow._wrap(v, ref, mask)                                                    # (the constructor refuses NaN and inf)


def _check_loss(loss, rec_sum, rec_count, what):
    with np.errstate(invalid='ignore', divide='ignore'):
        quotient = (rec_sum / rec_count).astype(np.float32)
    _same(_np(loss), quotient, what + " loss")


# ---- photometric and census -----------------------------------------------------------------------------------------------------------
# (variant, channels, uint8 images, fp16-stored flow)
SAMPLER_CONFIGS = [('finite', 3, False, False), ('finite', 3, True, False), ('finite', 3, False, True), ('finite', 1, False, False),
                   ('other', 3, False, False),
                   ('other', 1, False, False), ('img', 3, False, False), ('vectors', 3, False, False)]


def _sampler_inputs(h, w, ref, variant, c, u8, half, census=False):
    case = ls.sampler_case(h, w, ref, variant, c, half, census)
    img, other = (ls.as_uint8(case['img']), ls.as_uint8(case['other'])) if u8 else (case['img'], case['other'])
    return case, img, other


def _sampler_gradient(module, fn_name, grad_name, case, img, other, extra, rec_count):
    """The gradient with respect to the vectors: through autograd, or through the binding for an fp16 leaf"""
    sign = ls.sign_of(case['ref'])
    mask, ti, to = _t(case['mask']), _t(img), _t(other)
    if case['half']:
        scale = (_up().double() / rec_count).float()
        return _np(getattr(module, grad_name)(_t(case['a']), mask, ti, to, sign, *extra, scale))
    v = _t(case['a'], grad=True)
    loss = getattr(module, fn_name)(v, mask, ti, to, sign, *extra)
    assert loss.requires_grad
    loss.backward(_up())
    return _np(v.grad)


@gpu
@pytest.mark.parametrize("ref", ls.REFS)
@pytest.mark.parametrize("h,w", ls.SAMPLER_FRAMES, ids=lambda v: str(v))
def test_photometric(h, w, ref):
    from oflibpytorch_amd import _native, _photometric
    sign = ls.sign_of(ref)
    finite_run, worst = {}, 0.0
    for variant, c, u8, half in SAMPLER_CONFIGS:
        case, img, other = _sampler_inputs(h, w, ref, variant, c, u8, half)
        what = "photometric %d x %d '%s' %s C %d u8 %s half %s" % (h, w, ref, variant, c, u8, half)
        want = po.compute(case['a'], case['mask'], img, other, ref, EPS)
        g_want, big_a = po.grad(case['a'], case['mask'], img, other, ref, EPS, ls.UPSTREAM)
        known = want['known']
        rec, pmap = _photometric.flow_photometric(_t(case['a']), _t(case['mask']), _t(img), _t(other), sign, EPS, want_map=True)
        assert 'photometric' in _native.last_kernel_name()
        rec, pmap = _np(rec), _np(pmap)
        _same(pmap, want['map'], what)                                                    # (+0 where not known)
        _same64(rec[:, 0], want['records'][:, 0], what)
        _same64(rec[:, 2], want['records'][:, 2], what + " max")
        ls.check_record_sum(rec[:, 1], want['records'][:, 1], rec[:, 0])
        assert not rec[:, 3:].any(), what
        flow = _wrapped(_t(case['a']), ref, _t(case['mask']))
        _check_loss(flow.photometric(_t(img), _t(other), eps=EPS), rec[:, 1], rec[:, 0], what)
        _same(_np(flow.photometric_map(_t(img), _t(other), eps=EPS)), want['map'], what + " map of the API")
        got = _sampler_gradient(_photometric, 'photometric', 'flow_photometric_grad', case, img, other, (EPS,), _t(rec[:, 0]))
        assert 'flow_photometric_kernel' in _native.last_kernel_name()
        zero = ~np.broadcast_to(known[:, None], got.shape)
        ratio, share = ls.check_gradient(got, g_want, big_a, zero, po.ulp32, what)
        worst = max(worst, ratio)
        print("%s: sums %s max %s; gradient %.3f of its bound, %.3f of the known elements by class" % (what, rec[:, 1], rec[:, 2], ratio, share))
        for b, y, x in case['bad_vec']:
            assert not got[b, :, y, x].view(np.uint32).any() and not pmap[b, y, x].view(np.uint32), what
        key = (c, u8, half)
        if variant == 'finite':
            finite_run[key] = (rec, pmap, got)
            assert np.isfinite(pmap).all() and np.isfinite(got).all()
            for name in ls.BORDER:
                y, x = case['names'][name][0]
                assert np.all(got[:, :, y, x] != 0), (what, name)                           # the border pixels carry a gradient
        else:
            f_rec, f_map, f_grad = finite_run[key]
            touched = ls.sampler_touched(case)
            assert not touched[ls.CLEAN].any() and np.array_equal(rec[ls.CLEAN].view(np.uint64), f_rec[ls.CLEAN].view(np.uint64)), what
            assert np.array_equal(pmap.view(np.uint32)[~touched], f_map.view(np.uint32)[~touched]), what + " isolation"
            # (a vector that is not finite takes its pixel out of the count, and with it changes the scale of its image's gradient)
            assert variant == 'vectors' or np.array_equal(rec[:, 0], f_rec[:, 0])
            t2 = np.broadcast_to((touched | (rec[:, 0] != f_rec[:, 0])[:, None, None])[:, None], got.shape)
            assert np.array_equal(got.view(np.uint32)[~t2], f_grad.view(np.uint32)[~t2]), what + " isolation of the gradient"
    print("photometric %d x %d '%s': largest gradient error %.3f of the bound 2^-22 A + ulp32" % (h, w, ref, worst))


# (variant, patch, q, uint8, half, channels): the finite variant on every frame, the specials where a patch of 3 leaves most of the frame clean
def _census_configs(h, w):
    out = [('finite', 7, 0.4, False, False, 3), ('finite', 3, 1.0, False, False, 3), ('finite', 3, 0.4, False, False, 3),
           ('finite', 3, 0.4, True, False, 3), ('finite', 3, 0.4, False, True, 3), ('finite', 3, 1.0, False, False, 1),
           ('vectors', 3, 1.0, False, False, 3)]
    if (h, w) != (20, 28):
        out += [('other', 3, 1.0, False, False, 3), ('other', 3, 0.4, False, False, 3), ('other', 3, 1.0, False, False, 1),
                ('img', 3, 1.0, False, False, 3), ('img', 3, 0.4, False, False, 3)]
    return out


@gpu
@pytest.mark.parametrize("ref", ls.REFS)
@pytest.mark.parametrize("h,w", ls.SAMPLER_FRAMES + [ls.CENSUS_TILE_FRAME], ids=lambda v: str(v))
def test_census(h, w, ref):
    from oflibpytorch_amd import _census, _native
    sign = ls.sign_of(ref)
    finite_run, worst, worst_ulp = {}, 0.0, 0.0
    for variant, patch, q, u8, half, c in _census_configs(h, w):
        case, img, other = _sampler_inputs(h, w, ref, variant, c, u8, half, census=True)
        what = "census %d x %d '%s' %s patch %d q %g u8 %s half %s C %d" % (h, w, ref, variant, patch, q, u8, half, c)
        want = cen.compute(case['a'], case['mask'], img, other, ref, patch, cen.THRESH, cen.EPS, q)
        g_want, big_a = cen.grad(case['a'], case['mask'], img, other, ref, patch, cen.THRESH, cen.EPS, q, ls.UPSTREAM)
        known = want['known']
        extra = (patch, cen.THRESH, cen.EPS, q)
        rec, cmap = _census.flow_census(_t(case['a']), _t(case['mask']), _t(img), _t(other), sign, *extra, want_map=True)
        assert 'census' in _native.last_kernel_name()
        rec, cmap = _np(rec), _np(cmap)
        assert not cmap[~known].view(np.uint32).any(), what                                # exactly +0 where not known
        assert np.array_equal(sv.classes(cmap), sv.classes(want['map'])), what
        if q == 1.0:
            _same(cmap, want['map'], what)
        else:
            fin = np.isfinite(want['map'])
            ulps = np.abs(cmap[fin].astype(np.float64) - want['map'][fin]) / cen.ulp32(want['map'][fin])
            worst_ulp = max(worst_ulp, float(ulps.max()))
            assert np.all(ulps <= 1.0), (what, float(ulps.max()))
        _same64(rec[:, 0], want['records'][:, 0], what)
        _same64(rec[:, 3], want['records'][:, 3], what + " terms")
        # sum and max: those of the call's own map (the pow is within an ulp of the oracle's), by the rules of the records
        for i in range(N):
            vals = cmap[i][known[i]].astype(np.float64)
            assert rec[i, 2] == sv.record_max(vals), what
            ls.check_record_sum(rec[i, 1], sv.record_sum(vals), vals.size)
        assert not rec[:, 4:].any(), what
        flow = _wrapped(_t(case['a']), ref, _t(case['mask']))
        _check_loss(flow.census(_t(img), _t(other), patch=patch, q=q), rec[:, 1], rec[:, 0], what)
        got = _sampler_gradient(_census, 'census', 'flow_census_grad', case, img, other, extra, _t(rec[:, 0]))
        assert 'flow_census_grad_kernel' in _native.last_kernel_name()
        zero = ~np.broadcast_to(known[:, None], got.shape)
        ratio, share = ls.check_gradient(got, g_want, big_a, zero, cen.ulp32, what)
        worst = max(worst, ratio)
        print("%s: sums %s max %s; gradient %.3f of its bound, %.3f of the known elements by class" % (what, rec[:, 1], rec[:, 2], ratio, share))
        for b, y, x in case['bad_vec']:
            assert not got[b, :, y, x].view(np.uint32).any() and not cmap[b, y, x].view(np.uint32), what
        key = (patch, q, u8, half, c)
        if variant == 'finite':
            finite_run[key] = (rec, cmap, got)
            assert np.isfinite(cmap).all() and np.isfinite(got).all()
            for name in ls.BORDER:
                y, x = case['names'][name][0]
                assert np.all(got[:, :, y, x] != 0), (what, name)
        elif variant != 'vectors':
            f_rec, f_map, f_grad = finite_run[key]
            r = patch // 2
            touched, touched2 = ls.sampler_touched(case, r), ls.sampler_touched(case, 2 * r)
            assert not touched2[ls.CLEAN].any() and np.array_equal(rec[ls.CLEAN].view(np.uint64), f_rec[ls.CLEAN].view(np.uint64)), what
            assert np.array_equal(cmap.view(np.uint32)[~touched], f_map.view(np.uint32)[~touched]), what + " isolation"
            t2 = np.broadcast_to(touched2[:, None], got.shape)
            assert np.array_equal(got.view(np.uint32)[~t2], f_grad.view(np.uint32)[~t2]), what + " isolation of the gradient"
    print("census %d x %d '%s': q = 0.4 within %.2f ulp; largest gradient error %.3f of the bound 2^-22 A + ulp32" % (h, w, ref, worst_ulp, worst))


# ---- consistency: the named positions -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ref", ls.REFS)
@pytest.mark.parametrize("h,w", ls.SAMPLER_FRAMES, ids=lambda v: str(v))
def test_consistency(h, w, ref):
    from oflibpytorch_amd import _consistency, _native
    sign = ls.sign_of(ref)
    finite_run = {}
    for variant, half in (('finite', False), ('finite', True), ('other', False), ('vectors', False)):
        case = ls.sampler_case(h, w, ref, variant, 2, half)
        back = case['other'].astype(np.float16) if half else case['other']                 # (multiples of 1/128 below 16: exact)
        what = "consistency %d x %d '%s' %s half %s" % (h, w, ref, variant, half)
        want = co.check(case['a'], back, case['mask'], case['back_mask'], ref, CONS_ALPHA, CONS_BETA)
        err, cons, known, rec = _consistency.flow_consistency(_t(case['a']), _t(back), _t(case['mask']), _t(case['back_mask']), sign,
                                                              CONS_ALPHA, CONS_BETA)
        assert 'consistency' in _native.last_kernel_name()
        err, cons, known, rec = _np(err), _np(cons), _np(known), _np(rec)
        assert np.array_equal(known, want['known']) and np.array_equal(cons, want['consistent']), what
        _same(err, want['error'], what)
        _same64(rec[:, :2], want['records'][:, :2], what)
        _same64(rec[:, 3], want['records'][:, 3], what + " max")
        ls.check_record_sum(rec[:, 2], want['records'][:, 2], rec[:, 0])
        ls.check_record_sum(rec[:, 4], want['records'][:, 4], rec[:, 1])
        assert not rec[:, 5:].any(), what
        print("%s: known %s consistent %s sums %s max %s" % (what, rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]))
        for name in ls.INSIDE:
            y, x = case['names'][name][0]
            assert known[:, y, x].all(), (what, name)
        if variant == 'finite':
            finite_run[half] = (err, cons, known, rec)
        else:
            f_err, f_cons, f_known, f_rec = finite_run[half]
            touched = ls.sampler_touched(case)
            assert not touched[ls.CLEAN].any() and np.array_equal(rec[ls.CLEAN].view(np.uint64), f_rec[ls.CLEAN].view(np.uint64)), what
            for got_map, f_map in ((err.view(np.uint32), f_err.view(np.uint32)), (cons, f_cons), (known, f_known)):
                assert np.array_equal(got_map[~touched], f_map[~touched]), what + " isolation"


# ---- smoothness -----------------------------------------------------------------------------------------------------------------------
def _ulps32(got, want):
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


@gpu
@pytest.mark.parametrize("h,w", ls.SMOOTH_FRAMES, ids=lambda v: str(v))
def test_smoothness(h, w):
    from oflibpytorch_amd import _native, _smoothness
    finite_run, worst, worst_map = {}, 0.0, 0
    for variant in ls.SMOOTH_VARIANTS:
        case = ls.smoothness_case(h, w, variant)
        runs = ls.smooth_runs(variant) +([(o, 0.0, True) for o in (1, 2)] if variant == 'finite' else [])
        for order, alpha, with_img in runs:
            what = "smoothness %d x %d %s order %d alpha %g image %s" % (h, w, variant, order, alpha, with_img)
            img = case['img'] if with_img else None
            want = so.compute(case['flow'], case['mask'], img, order, alpha, EPS)
            g_want, big_a, read = so.grad(case['flow'], case['mask'], img, order, alpha, EPS, ls.UPSTREAM)
            ti = None if img is None else _t(img)
            rec, smap = _smoothness.flow_smoothness(_t(case['flow']), _t(case['mask']), ti, order, alpha, EPS, want_map=True)
            assert 'smoothness' in _native.last_kernel_name()
            rec, smap = _np(rec), _np(smap)
            bearing = want['x']['ok'] | want['y']['ok']
            assert not smap[~bearing].view(np.uint32).any(), what                          # exactly +0 where no term is valid
            wrec = want['records']
            _same64(rec[:, :2], wrec[:, :2], what)
            if not with_img:
                _same(smap, want['map'], what)                                             # bit for bit
                _same64(rec[:, 4], wrec[:, 4], what + " max")
                for k in (2, 3):
                    ls.check_record_sum(rec[:, k], wrec[:, k], wrec[:, k - 2])
            else:
                # the weight is the float64 exp of device and NumPy rounded once: 4 ulp on the map, 2 on the max (tests/test_gpu_smoothness.py)
                assert np.array_equal(sv.classes(smap), sv.classes(want['map'])), (what, sv.describe(smap, want['map']))
                fin = np.isfinite(want['map'])
                d = _ulps32(smap[fin], want['map'][fin])
                worst_map = max(worst_map, int(d.max()))
                assert d.max() <= 4, (what, int(d.max()))
                for k in (2, 3):
                    ls.check_record_sum(rec[:, k], wrec[:, k], np.ones(N), 2.0 ** -22 + wrec[:, k - 2] * 2.0 ** -52)
                assert np.array_equal(sv.classes(rec[:, 4]), sv.classes(wrec[:, 4])), what
                fm = np.isfinite(wrec[:, 4])
                assert _ulps32(rec[fm, 4].astype(np.float32), wrec[fm, 4].astype(np.float32)).max() <= 2, what
            flow = _wrapped(_t(case['flow']), 't', _t(case['mask']))
            _check_loss(flow.smoothness(ti, order=order, alpha=alpha, eps=EPS), rec[:, 2] + rec[:, 3], rec[:, 0] + rec[:, 1], what)
            v = _t(case['flow'], grad=True)
            loss = _smoothness.smoothness(v, _t(case['mask']), ti, order, alpha, EPS)
            loss.backward(_up())
            assert 'flow_smoothness_kernel' in _native.last_kernel_name()
            got = _np(v.grad)
            zero = ~np.broadcast_to(read[:, None], got.shape)
            ratio, share = ls.check_gradient(got, g_want.astype(np.float64), big_a, zero, so.ulp32, what)
            worst = max(worst, ratio)
            print("%s: sums %s %s max %s; gradient %.3f of its bound, %.3f by class" % (what, rec[:, 2], rec[:, 3], rec[:, 4], ratio, share))
            key = (order, alpha, with_img)
            if variant == 'finite':
                finite_run[key] = (rec, smap, got)
                assert np.isfinite(smap).all() and np.isfinite(got).all()
            else:
                f_rec, f_map, f_grad = finite_run[key]
                touched = ls.dilate(case['hit'], order)
                assert not touched[ls.CLEAN].any() and np.array_equal(rec[ls.CLEAN].view(np.uint64), f_rec[ls.CLEAN].view(np.uint64)), what
                assert np.array_equal(smap.view(np.uint32)[~touched], f_map.view(np.uint32)[~touched]), what + " isolation"
                t2 = np.broadcast_to(touched[:, None], got.shape)
                assert np.array_equal(got.view(np.uint32)[~t2], f_grad.view(np.uint32)[~t2]), what + " isolation of the gradient"
    print("smoothness %d x %d: map within %d ulp with an image; largest gradient error %.3f of the bound 2^-22 A + ulp32" % (h, w, worst_map, worst))


# ---- error_stats and epe --------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("h,w", ls.ERROR_FRAMES, ids=lambda v: str(v))
def test_error_stats(h, w):
    from oflibpytorch_amd import _native
    finite_run, worst = None, 0.0
    thr = feo.DEFAULT_THRESHOLDS
    for variant in ls.ERROR_VARIANTS:
        case = ls.error_case(h, w, variant)
        what = "error_stats %d x %d %s" % (h, w, variant)
        want = feo.score(case['est'], case['gt'], case['est_mask'], case['gt_mask'], thr)
        ops = lambda grad=False: (_t(case['est'], grad), _t(case['gt']), _t(case['est_mask']), _t(case['gt_mask']))
        rec, emap = _native.flow_error(*ops(), thr, True)
        assert 'flow_error' in _native.last_kernel_name()
        rec, emap = _np(rec), _np(emap)
        _same(emap, want['map'], what)                                                     # (+0 where not valid)
        _same64(rec[:, 0], want['count'].astype(np.float64), what)
        _same64(rec[:, 2], want['max'], what + " max")
        # a NaN error passes no threshold and no Fl test; its pixel is binned by the speed of the ground truth, NaN in the last bin
        _same64(rec[:, 3:3 + len(thr)], want['n_over'].astype(np.float64), what + " thresholds")
        _same64(rec[:, 7], want['n_fl'].astype(np.float64), what + " fl")
        _same64(rec[:, 8:11], want['speed_count'].astype(np.float64), what + " speed bins")
        ls.check_record_sum(rec[:, 1], want['sum'], rec[:, 0])
        ls.check_record_sum(rec[:, 11:14], want['speed_sum'], rec[:, 8:11])
        assert not rec[:, 14:].any(), what
        est, gt, em, gm = ops(True)
        loss = _native.flow_epe(est, gt, em, gm)
        _check_loss(loss, rec[:, 1], rec[:, 0], what)
        loss.backward(_up())
        assert 'flow_epe_grad_kernel' in _native.last_kernel_name()
        got = _np(est.grad)
        g_want = feo.epe_grad(case['est'], case['gt'], case['est_mask'], case['gt_mask'], np.asarray(ls.UPSTREAM, np.float32) / rec[:, 0])
        # exactly +0 where the pixel is not valid or its float32 e is 0 or NaN
        live = feo.valid_of(case['est_mask'].shape, case['est_mask'], case['gt_mask']) & (feo.pixel_terms(case['est'], case['gt'])[2] > 0)
        zero = ~np.broadcast_to(live[:, None], got.shape)
        assert not got[zero].view(np.uint32).any() and not g_want[zero].any(), what
        by_class = ~np.isfinite(g_want)
        assert np.array_equal(sv.classes(got)[by_class], sv.classes(g_want)[by_class]), what
        rest = ~zero & ~by_class
        ulp = np.spacing(np.abs(g_want[rest]).astype(np.float32)).astype(np.float64)
        ratio = float((np.abs(got[rest].astype(np.float64) - g_want[rest]) / ulp).max())
        worst = max(worst, ratio)
        assert ratio <= 4.0, (what, ratio)
        print("%s: sum %s max %s; gradient within %.3f ulp, %d elements by class" % (what, rec[:, 1], rec[:, 2], ratio, by_class.sum()))
        if variant == 'finite':
            finite_run = (rec, emap, got)
        else:
            f_rec, f_map, f_grad = finite_run
            hit = case['hit']
            assert not hit[ls.CLEAN].any() and np.array_equal(rec[ls.CLEAN].view(np.uint64), f_rec[ls.CLEAN].view(np.uint64)), what
            assert np.array_equal(emap.view(np.uint32)[~hit], f_map.view(np.uint32)[~hit]), what + " isolation"
            h2 = np.broadcast_to(hit[:, None], got.shape)
            assert np.array_equal(got.view(np.uint32)[~h2], f_grad.view(np.uint32)[~h2]), what + " isolation of the gradient"
    print("error_stats %d x %d: largest gradient error %.3f ulp" % (h, w, worst))
