"""CPU tier of tests/loss_specials.py: the inputs of tests/test_gpu_loss_specials.py are what their names say, every case shows every
class of result (so that no GPU test passes on an empty set), the oracles are total on them, the oracle's gradient on the finite variant
is torch's float64 autograd at the named border pixels too, and the share of gradient elements that can be checked by class only stays
under a quarter.  For SSIM and the cost volume also: the comparison functions of the GPU tier pass on the oracles put in the bindings'
place and fail on a map element one ulp up, a moved gradient element and a NaN where a +0 is due.  Runs without a GPU."""
import functools

import numpy as np
import pytest
import torch

import census_oracle as cen
import consistency_oracle as co
import cost_volume_oracle as cvo
import flow_error_oracle as feo
import grad_oracle64 as go
import loss_specials as ls
import photometric_oracle as po
import smoothness_oracle as so
import special_values as sv
import ssim_oracle as sso
from test_photometric_host import _torch_loss

FRAMES = ls.SAMPLER_FRAMES
CAP = 0.25
CONS_ALPHA, CONS_BETA = 1.0, 0.5


def _classes_seen(x):
    return set(np.unique(sv.classes(x)).tolist())


@functools.lru_cache(maxsize=None)
def _photo(h, w, ref, variant):
    c = ls.sampler_case(h, w, ref, variant)
    return po.compute(c['a'], c['mask'], c['img'], c['other'], ref), po.grad(c['a'], c['mask'], c['img'], c['other'], ref, upstream=ls.UPSTREAM)


@functools.lru_cache(maxsize=None)
def _census(h, w, ref, variant):
    c = ls.sampler_case(h, w, ref, variant, census=True)
    return (cen.compute(c['a'], c['mask'], c['img'], c['other'], ref, 3),
            cen.grad(c['a'], c['mask'], c['img'], c['other'], ref, 3, upstream=ls.UPSTREAM))


def _share(want, big_a, live):
    """Per image: the share of the elements of `live` [N,H,W] whose expected gradient (as float32) or A is not finite"""
    with np.errstate(over='ignore', invalid='ignore'):
        by_class = (~np.isfinite(want.astype(np.float32)) | ~np.isfinite(big_a)) & live[:, None]
    return [float(by_class[i].sum()) / max(2 * int(live[i].sum()), 1) for i in range(ls.N)]


# ---- the oracles' record rules --------------------------------------------------------------------------------------------------------
def test_record_sum_and_max_rules():
    assert sv.record_sum([]) == 0.0 and sv.record_max([]) == 0.0
    assert sv.record_sum([0.1] * 10) == 1.0 and sv.record_max([0.5, 2.0, 1.0]) == 2.0        # fsum: exact, rounded once
    assert np.isnan(sv.record_sum([1.0, np.nan, np.inf])) and sv.record_sum([1.0, np.inf]) == np.inf
    assert sv.record_max([1.0, np.nan, 3.0]) == 3.0 and sv.record_max([np.nan]) == 0.0 and sv.record_max([np.nan, np.inf, 2.0]) == np.inf


def test_warp_case_defaults_are_unchanged_by_the_new_parameters():
    """finite=True draws the same numbers: the flow is the same and the source differs exactly where a special was planted"""
    spec, fin = sv.warp_case(2, 20, 28, 3, seed=5), sv.warp_case(2, 20, 28, 3, seed=5, finite=True)
    assert np.array_equal(spec['flow'], fin['flow']) and spec['names'] == fin['names'] and spec['planted'] == fin['planted']
    assert np.isfinite(fin['src']).all() and not (fin['src'] == sv.FLT_MAX).any()
    finite_there = np.isfinite(spec['src']) & (np.abs(spec['src']) < 1e30) & (np.abs(spec['src']) > 1e-30)
    assert np.array_equal(spec['src'][finite_there], fin['src'][finite_there])
    few = sv.warp_case(2, 20, 28, 3, seed=5, sprinkle=0.0, plant_names=('on_integer',))
    assert len(few['planted']) == 1 and np.isnan(few['src'][:, 0][:, few['planted'][0][0], few['planted'][0][1]]).all()


# ---- the named positions --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", ls.REFS)
@pytest.mark.parametrize("h,w", FRAMES)
def test_every_named_position_is_what_its_name_says(h, w, ref):
    c = ls.sampler_case(h, w, ref, 'other')
    assert set(c['names']) == set(ls.NAMES) and len(c['names']['flow_extreme']) == len(sv.WARP_FLOW_EXTREMES)
    sx, sy = go.warp_positions(c['a'], ls.N, ls.sign_of(ref))
    t = go.warp_taps(c['a'], ls.N, ls.sign_of(ref))
    ok, wgt, idx = t.ok, t.wgt, t.idx                       # taps nw, ne, sw, se
    for name in ls.OUTSIDE:
        # -1 and the size need not come back exactly (special_values.sample_coord): within an ulp of them, and no tap has weight
        (y, x), (ay, ax) = c['names'][name][0], c['aimed'][name]
        assert np.all(np.abs(sx[:, y, x] - ax) < 1e-5) and np.all(np.abs(sy[:, y, x] - ay) < 1e-5), name
        assert all(np.all(np.where(ok[j][:, y, x], wgt[j][:, y, x], 0.0) < 1e-5) for j in range(4)), name
    for name in ls.INSIDE:
        (y, x), (ay, ax) = c['names'][name][0], c['aimed'][name]
        # the integer aimed at comes back from the sampler's own arithmetic as that integer
        assert np.all(sx[:, y, x] == ax) and np.all(sy[:, y, x] == ay), name
        assert sv.sample_coord(np.float32(ax), w) == ax and sv.sample_coord(np.float32(ay), h) == ay, name
        inside_x, inside_y = 0 <= ax < w, 0 <= ay < h
        east_in, south_in = 0 <= ax + 1 < w, 0 <= ay + 1 < h
        assert np.all(ok[0][:, y, x] == (inside_x and inside_y)) and np.all(ok[1][:, y, x] == (east_in and inside_y)), name
        assert np.all(ok[2][:, y, x] == (inside_x and south_in)) and np.all(ok[3][:, y, x] == (east_in and south_in)), name
        assert np.all(wgt[0][:, y, x] == 1.0) and all(np.all(wgt[j][:, y, x] == 0.0) for j in (1, 2, 3)), name   # fraction exactly 0
    for name, (dy, dx) in (('last_row', (1, 0)), ('last_col', (0, 1)), ('last_corner', (1, 1))):
        ay, ax = c['aimed'][name]
        assert (ay + dy == h or not dy) and (ax + dx == w or not dx), name
    assert c['aimed']['x_m1'][1] == -1 and c['aimed']['y_m1'][0] == -1 and c['aimed']['x_size'][1] == w and c['aimed']['y_size'][0] == h
    assert c['aimed']['x_0'][1] == 0 and c['aimed']['x_last'][1] == w - 1
    # the weight-0 source pixels hold a special and their named reader reads them through a tap of weight 0 only
    readers = {'weight0_east': 1, 'weight0_south': 2, 'x_m1': 1, 'y_m1': 2}
    assert len(c['weight0']) == len(readers)
    for (name, tap), (py, px) in zip(readers.items(), c['weight0']):
        y, x = c['names'][name][0]
        assert not np.isfinite(c['other'][ls.MIXED, :, py, px]).any(), name
        for j in range(4):
            hits = ok[j][:, y, x] & (idx[j][:, y, x] == py * w + px)
            if name.startswith('weight0'):
                assert np.all(hits == (j == tap)) and np.all(wgt[tap][:, y, x] == 0.0), (name, j)
            else:
                assert np.all(wgt[j][:, y, x][hits] < 1e-5), (name, j)                       # (an ulp inside the frame at most)
    # the extreme vectors sit where the case says, in every image
    for i, (e, (y, x)) in enumerate(zip(sv.WARP_FLOW_EXTREMES, c['names']['flow_extreme'])):
        assert np.all(c['a'][:, i % 2, y, x] == np.float32(ls.sign_of(ref)) * e), (i, e)     # ('s': the case's flow negated)


# ---- coverage: photometric, census, consistency ---------------------------------------------------------------------------------------
def _assert_record_classes(rec_sum, rec_max, can_be_inf):
    assert np.isnan(rec_sum[ls.MIXED]) and np.isnan(rec_sum[ls.NAN_ONLY]) and np.isfinite(rec_sum[ls.CLEAN])
    assert np.isfinite(rec_max[ls.NAN_ONLY]) and rec_max[ls.NAN_ONLY] > 0                   # a NaN sum next to a finite maximum
    if can_be_inf:
        assert rec_sum[ls.MAX_ONLY] == np.inf and rec_max[ls.MAX_ONLY] == np.inf            # +inf is taken, nothing is NaN
        assert rec_max[ls.MIXED] == np.inf                                                 # a NaN sum next to an infinite maximum


@pytest.mark.parametrize("ref", ls.REFS)
@pytest.mark.parametrize("h,w", FRAMES)
def test_photometric_cases_show_every_class(h, w, ref):
    """A record sum of +inf next to a FINITE maximum cannot occur in any family: the terms are float32 and the sums float64, so a sum
    is +inf only through a term of +inf, which the maximum takes.  What is seen instead: NaN sum / finite max, NaN sum / +inf max,
    +inf sum / +inf max, and the clean neighbour."""
    clean = _photo(h, w, ref, 'finite')[0]
    for variant in ls.VARIANTS:
        c = ls.sampler_case(h, w, ref, variant)
        res, (want, big_a) = _photo(h, w, ref, variant)
        known = res['known']
        for name in ls.INSIDE:
            assert all(known[:, y, x].all() for y, x in c['names'][name]), (variant, name)
        for name in ls.OUTSIDE:
            assert not any(known[:, y, x].any() for y, x in c['names'][name]), (variant, name)
        assert np.array_equal(known[ls.CLEAN], clean['known'][ls.CLEAN])
        assert np.array_equal(res['map'][ls.CLEAN].view(np.uint32), clean['map'][ls.CLEAN].view(np.uint32))
        share = _share(want, big_a, known)
        print("photometric %d x %d '%s' %s: known %s, gradient elements checked by class %s" % (h, w, ref, variant,
                                                                                               known.sum((1, 2)).tolist(), np.round(share, 3)))
        assert max(share) <= CAP
        if variant in ('other', 'img'):
            assert _classes_seen(res['map'][ls.MIXED][known[ls.MIXED]]) >= {0, 1, 2}
            _assert_record_classes(res['records'][:, 1], res['records'][:, 2], True)
            touched = ls.sampler_touched(c)
            assert 0 < (touched & known).sum() < 0.3 * known.sum() and not touched[ls.CLEAN].any()
            same = sv.same_bits(res['map'], clean['map'])
            assert same[~touched].all() and not same[touched & known].all()
        if variant == 'vectors':
            assert len(c['bad_vec']) == 3 * len(ls.VECTOR_PLANTS) and not any(known[b, y, x] for b, y, x in c['bad_vec'])
            assert sum(bool(clean['known'][b, y, x]) for b, y, x in c['bad_vec']) >= 3       # (they were known before)
            assert np.isfinite(res['records']).all() and np.isfinite(want).all()
        if variant == 'finite':
            assert np.isfinite(res['map']).all() and np.isfinite(want).all() and max(share) == 0
            for name in ls.BORDER:
                y, x = c['names'][name][0]
                assert np.all(want[:, :, y, x] != 0), name                                  # the one-sided derivative is not zero


@pytest.mark.parametrize("ref", ls.REFS)
@pytest.mark.parametrize("h,w", FRAMES + [ls.CENSUS_TILE_FRAME])
def test_census_cases_show_every_class(h, w, ref):
    """The census penalty is NaN or finite, never infinite: every term s / (thresh + s) is at most 1 or NaN (an infinite grey
    difference makes the soft sign inf / inf).  So the classes are finite and NaN, and the record is NaN next to a finite maximum."""
    clean = _census(h, w, ref, 'finite')[0]
    for variant in ls.VARIANTS:
        if (h, w) == (20, 28) and variant in ('other', 'img'):
            continue                                                                         # (3 x 49 contaminated centres fill the frame)
        c = ls.sampler_case(h, w, ref, variant, census=True)
        res, (want, big_a) = _census(h, w, ref, variant)
        known = res['known']
        assert all(known[:, y, x].all() for name in ls.INSIDE for y, x in c['names'][name]), variant
        share = _share(want, big_a, known)
        print("census %d x %d '%s' %s: known %s, gradient elements checked by class %s" % (h, w, ref, variant, known.sum((1, 2)).tolist(),
                                                                                         np.round(share, 3)))
        assert max(share) <= CAP
        assert _classes_seen(res['map']) <= {0, 1} and _classes_seen(res['records'][:, 2]) == {0}
        if variant in ('other', 'img'):
            assert all(np.isnan(res['records'][i, 1]) for i in (ls.MIXED, ls.MAX_ONLY, ls.NAN_ONLY)) and np.isfinite(res['records'][ls.CLEAN, 1])
            touched = ls.sampler_touched(c, 1)
            same = sv.same_bits(res['map'], clean['map'])
            assert same[~touched].all() and not same[touched & known].all() and not touched[ls.CLEAN].any()
            grad_touched = ls.sampler_touched(c, 2)
            assert np.isfinite(want[~np.broadcast_to(grad_touched[:, None], want.shape)]).all()
            if (h, w) == ls.CENSUS_TILE_FRAME:
                # the contaminated patches straddle the four tiles that meet at (16, 64)
                nan_map = np.isnan(res['map'][ls.MIXED])
                assert nan_map[:16, :64].any() and nan_map[:16, 64:].any() and nan_map[16:, :64].any()
                if variant == 'img':                                                         # (the fourth tile is this one pixel)
                    assert nan_map[16, 64] or not known[ls.MIXED, 16, 64]
        else:
            assert np.isfinite(res['records']).all() and np.isfinite(want).all()
        if variant == 'finite':
            for name in ls.BORDER:
                y, x = c['names'][name][0]
                assert np.all(want[:, :, y, x] != 0), name


@pytest.mark.parametrize("ref", ls.REFS)
@pytest.mark.parametrize("h,w", FRAMES)
def test_consistency_cases_show_every_class(h, w, ref):
    clean = None
    for variant in ('finite', 'other', 'vectors'):
        c = ls.sampler_case(h, w, ref, variant, c=2)
        res = co.check(c['a'], c['other'], c['mask'], c['back_mask'], ref, CONS_ALPHA, CONS_BETA)
        clean = res if variant == 'finite' else clean
        known = res['known']
        assert all(known[:, y, x].all() for name in ls.INSIDE for y, x in c['names'][name]), variant
        assert not any(known[:, y, x].any() for name in ls.OUTSIDE for y, x in c['names'][name]), variant
        assert all(0 < res['records'][i, 1] < res['records'][i, 0] for i in range(ls.N))        # consistent and inconsistent pixels
        if variant == 'other':
            assert np.array_equal(known, clean['known'])                                      # `known` never reads back's vectors
            assert _classes_seen(res['error'][ls.MIXED][known[ls.MIXED]]) >= {0, 1, 2}
            _assert_record_classes(res['records'][:, 2], res['records'][:, 3], True)
            touched = ls.sampler_touched(c)
            same = sv.same_bits(res['error'], clean['error'])
            assert same[~touched].all() and not same[touched & known].all()
        else:
            assert np.isfinite(res['records']).all()


# ---- coverage: smoothness, error_stats ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", ls.SMOOTH_FRAMES)
def test_smoothness_cases_show_every_class(h, w):
    assert (w % 4 != 0) == ((h, w) == ls.SMOOTH_FRAMES[0]) and h > so.TH and w > so.TW
    for variant in ls.SMOOTH_VARIANTS:
        c = ls.smoothness_case(h, w, variant)
        f = ls.smoothness_case(h, w, 'finite')
        assert np.array_equal(c['mask'], f['mask']) and not c['hit'][ls.CLEAN].any()
        if variant != 'finite':
            for y, x in ls.smooth_plants(h, w):
                assert c['hit'][ls.MIXED, y, x] and c['mask'][:, y, x].all()
        for order, alpha, with_img in ls.smooth_runs(variant):
            img = c['img'] if with_img else None
            res = so.compute(c['flow'], c['mask'], img, order, alpha)
            g, big_a, read = so.grad(c['flow'], c['mask'], img, order, alpha, upstream=ls.UPSTREAM)
            share = _share(g.astype(np.float64), big_a, read)
            print("smoothness %d x %d %s order %d alpha %g image %s: map classes %s, sums %s, max %s, by class %s" % (
                h, w, variant, order, alpha, with_img, np.bincount(sv.classes(res['map']).ravel(), minlength=3).tolist(),
                res['records'][:, 2].tolist(), res['records'][:, 4].tolist(), np.round(share, 3)))
            assert max(share) <= CAP
            clean = so.compute(f['flow'], f['mask'], f['img'] if with_img else None, order, alpha)
            touched = ls.dilate(c['hit'], order)
            assert sv.same_bits(res['map'], clean['map'])[~touched].all()
            assert np.array_equal(res['records'][ls.CLEAN], clean['records'][ls.CLEAN])
            if variant == 'vectors':
                assert _classes_seen(res['map'][ls.MIXED]) >= {0, 1, 2}
                _assert_record_classes(res['records'][:, 2], res['records'][:, 4], True)
            at = 40 if order == 1 else 41                       # the x term whose image difference reads (2, 40) and a finite pixel
            if variant == 'both':
                # weight exactly 0 on an infinite r (alpha > 0), 0 * inf in the weight itself (alpha = 0): NaN both ways
                assert np.isnan(res['x']['t'][ls.MIXED, 2, at]) and np.isnan(res['records'][ls.MIXED, 2])
                assert np.isinf(res['x']['dv'][ls.MIXED, 2, at])
            if variant in ('image', 'both') and alpha > 0:
                assert res['x']['w'][ls.MIXED, 2, at] == 0.0 and res['x']['ok'][ls.MIXED, 2, at]      # +inf next to a finite pixel
            if variant in ('image', 'both') and alpha == 0:
                assert np.isnan(res['x']['w'][ls.MIXED, 2, at])


@pytest.mark.parametrize("h,w", ls.ERROR_FRAMES)
def test_error_cases_show_every_class(h, w):
    clean = None
    for variant in ls.ERROR_VARIANTS:
        c = ls.error_case(h, w, variant)
        res = feo.score(c['est'], c['gt'], c['est_mask'], c['gt_mask'])
        clean = res if variant == 'finite' else clean
        assert np.array_equal(res['count'], clean['count']) and (res['speed_count'] > 0).all()
        assert sv.same_bits(res['map'], clean['map'])[~c['hit']].all()
        if variant == 'finite':
            assert np.isfinite(res['records']).all()
            # a maximum taken over every pixel, the ones that do not count included, would be larger
            e_all = feo.pixel_terms(c['est'], c['gt'])[2]
            assert all(e_all[i][~(c['est_mask'][i] & c['gt_mask'][i])].max() > res['max'][i] for i in range(ls.N))
            continue
        assert c['hit'][ls.MIXED].sum() == 11 and not c['hit'][ls.CLEAN].any()
        assert _classes_seen(res['map'][ls.MIXED]) >= {0, 1, 2}
        _assert_record_classes(res['sum'], res['max'], True)
        assert np.array_equal(res['records'][ls.CLEAN], clean['records'][ls.CLEAN])
        # a NaN error passes no threshold and no Fl test: the counts of the NaN-only image can only fall
        assert np.all(res['n_over'][ls.NAN_ONLY] <= clean['n_over'][ls.NAN_ONLY]) and res['n_fl'][ls.NAN_ONLY] <= clean['n_fl'][ls.NAN_ONLY]
        g = feo.epe_grad(c['est'], c['gt'], c['est_mask'], c['gt_mask'], np.asarray(ls.UPSTREAM) / res['count'])
        assert _classes_seen(g[ls.MIXED]) >= {0, 1} and np.isfinite(g[ls.MAX_ONLY]).all() and np.isfinite(g[ls.CLEAN]).all()
        assert (~np.isfinite(g)).sum() <= 0.01 * g.size


# ---- the inputs tell a wrong kernel from a right one ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", ls.REFS)
@pytest.mark.parametrize("h,w", FRAMES)
def test_sampler_inputs_would_show_a_wrong_tap_rule_or_a_wrong_maximum(h, w, ref):
    """What a kernel that departs from its section would change, shown on the finite variant without running one.  (a) A tap that
    leaves the frame at fraction 0 counted as a gradient term: a kernel reads it at the offset clamped into the plane (row 0 for a
    south tap of the last row, column 0 for an east tap of the last column); those samples and the pixel's d are not 0, so its
    gradient would move.  (b) A record maximum taken over every pixel, not the known ones: in every image a pixel that is not known
    (the named ones outside the frame, whose `img` is 1024) holds a larger rho than every known one."""
    c = ls.sampler_case(h, w, ref, 'finite')
    res = _photo(h, w, ref, 'finite')[0]
    for name, (ty, tx) in (('last_row', (0, None)), ('last_col', (None, 0)), ('last_corner', (0, 0))):
        (y, x), (ay, ax) = c['names'][name][0], c['aimed'][name]
        clamped = c['other'][:, :, ay if ty is None else ty, ax if tx is None else tx]
        assert np.all(clamped != 0) and np.all(res['d'][:, :, y, x] != 0), name
    ee = np.float32(1e-3) * np.float32(1e-3)
    rho_all = np.sqrt(res['d'] * res['d'] + ee).sum(1) / np.float32(3)
    over = [float(np.nanmax(rho_all[i][~res['known'][i]])) > res['records'][i, 2] for i in range(ls.N)]      # (fmaxf skips a NaN)
    assert all(over), over


@pytest.mark.parametrize("h,w", ls.SMOOTH_FRAMES)
def test_smoothness_inputs_would_show_an_unread_halo_validity_byte(h, w):
    """Column 128 is the right halo column of the tiles of columns 0 .. 127 and column 127 the left halo of their neighbours (backward
    pass).  In some image a pixel of each is masked out next to valid pixels of its row: a kernel that took a halo pixel inside the frame
    for valid would count an x term more."""
    mask = ls.smoothness_case(h, w, 'finite')['mask']
    assert (~mask[:, :, so.TW] & mask[:, :, so.TW - 1]).any() and (~mask[:, :, so.TW - 1] & mask[:, :, so.TW]).any()
    assert (~mask[:, so.TH, :] & mask[:, so.TH - 1, :]).any()                                # (and of the row below a tile)


# ---- the oracle's gradient on the finite variant is the float64 derivative, border pixels included ---------------------------------
@pytest.mark.parametrize("ref", ls.REFS)
@pytest.mark.parametrize("h,w", FRAMES)
def test_oracle_gradient_is_autograd_at_the_named_border_pixels(h, w, ref):
    """torch's float64 autograd of the same expression on the pixels whose float32 sample position is exact (the named ones are, by
    construction; elsewhere the two may floor differently): the taps that leave the frame at fraction 0 contribute nothing."""
    c = ls.sampler_case(h, w, ref, 'finite')
    sign = ls.sign_of(ref)
    res, (got, big_a) = _photo(h, w, ref, 'finite')
    a = c['a']
    sx, sy = go.warp_positions(a, ls.N, sign)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    exact = (sx.astype(np.float64) == xs - sign * a[:, 0].astype(np.float64)) & (sy.astype(np.float64) == ys - sign * a[:, 1].astype(np.float64))
    u = torch.from_numpy(a).double().requires_grad_(True)
    loss = _torch_loss(u, torch.from_numpy(res['known']), torch.from_numpy(c['img']).double(), torch.from_numpy(c['other']).double(), sign,
                       float(np.float32(1e-3)))
    (loss * torch.tensor(ls.UPSTREAM, dtype=torch.float64)).sum().backward()
    want = u.grad.numpy()
    sel = np.broadcast_to((exact & res['known'])[:, None], want.shape)
    scale = np.abs(want[sel]).max()
    err = np.abs(got - want)[sel].max()
    print("%d x %d '%s': %d of %d known pixels exact, max |oracle - autograd| = %.3e of a gradient scale %.3e" % (
        h, w, ref, (exact & res['known']).sum(), res['known'].sum(), err, scale))
    assert err <= 1e-6 * scale and (exact & res['known']).sum() > 0.1 * res['known'].sum()
    for name in ls.BORDER + ('on_integer', 'weight0_east', 'weight0_south', 'x_0', 'x_last'):
        y, x = c['names'][name][0]
        assert exact[:, y, x].all() and res['known'][:, y, x].all(), name
        assert np.all(np.abs(got[:, :, y, x] - want[:, :, y, x]) <= 1e-6 * scale), name


# ---- SSIM ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ssim(h, w, window, ref, variant):
    c = ls.ssim_case(h, w, ref, variant)
    res = sso.compute(c['a'], c['mask'], c['img'], c['other'], ref, window)
    return res, sso.grad(c['a'], c['mask'], c['img'], c['other'], ref, window, upstream=ls.UPSTREAM, res=res)


def _class_share(want, big_a, known):
    """Per image: the share of the non-zero gradient elements of the known pixels that `check_gradient` holds by class only"""
    with np.errstate(over='ignore', invalid='ignore'):
        by_class = (~np.isfinite(want.astype(np.float32)) | ~np.isfinite(big_a)) & known[:, None]
    live = ((want != 0) | by_class) & known[:, None]
    return [float(by_class[i].sum()) / max(int(live[i].sum()), 1) for i in range(ls.N)]


@pytest.mark.parametrize("ref", ls.REFS)
@pytest.mark.parametrize("h,w,window", ls.SSIM_FRAMES)
def test_ssim_cases_show_every_class_under_the_cap(h, w, window, ref):
    """The SSIM penalty is NaN or in [0, 1], never infinite: the record is NaN next to a finite maximum in all three special images (with
    FLT_MAX the float32 forward forms inf - inf; the float64 backward does not overflow and stays finite).  Images on the scale 0 .. 1
    with the specials planted after the scaling; the class-only share of the non-zero gradient elements stays under the cap."""
    r = window // 2
    clean, (clean_g, _) = _ssim(h, w, window, ref, 'finite')
    fin = ls.ssim_case(h, w, ref, 'finite')
    assert fin['img'].max() <= 4.0 and fin['other'].max() < 1.0 and fin['img'][fin['img'] < 4.0].max() < 1.0
    assert np.array_equal(fin['img'] * ls.SCALE, ls.sampler_case(h, w, ref, 'finite', census=True)['img'])          # exact
    for variant in ls.SSIM_VARIANTS:
        c = ls.ssim_case(h, w, ref, variant)
        res, (want, big_a) = _ssim(h, w, window, ref, variant)
        known = res['known']
        assert all(known[:, y, x].all() for name in ls.INSIDE for y, x in c['names'][name]), variant
        assert not any(known[:, y, x].any() for name in ls.OUTSIDE for y, x in c['names'][name]), variant
        share = _class_share(want, big_a, known)
        print("ssim %d x %d window %d '%s' %s: known %s, non-zero gradient elements checked by class %s" % (
            h, w, window, ref, variant, known.sum((1, 2)).tolist(), np.round(share, 3)))
        assert max(share) <= CAP
        assert _classes_seen(res['map']) <= {0, 1} and _classes_seen(res['records'][:, 2]) == {0}
        assert np.array_equal(res['map'][ls.CLEAN].view(np.uint32), clean['map'][ls.CLEAN].view(np.uint32))
        assert np.array_equal(res['records'][ls.CLEAN], clean['records'][ls.CLEAN])
        for i in range(ls.N):                                                                  # the record follows the rule of 3.16
            vals = res['map'][i][known[i]].astype(np.float64)
            assert res['records'][i, 2] == sv.record_max(vals)
            assert np.array_equal(res['records'][i, 1], sv.record_sum(vals), equal_nan=True)
        if variant in ('other', 'img'):
            hit = c['src_hit'] if variant == 'other' else c['img_hit']
            assert hit[ls.MIXED].sum() >= 3 and not hit[ls.CLEAN].any()                         # the named plants, no sprinkle
            if (h, w) == ls.CENSUS_TILE_FRAME:                                                  # (the last corner is one of the four)
                assert hit[ls.MIXED].sum() == (6 if variant == 'other' else 7) and all(hit[ls.MIXED, y, x] for y, x in ls.CENSUS_TILE_PIXELS)
            else:
                assert hit[ls.MIXED].sum() == 3
            arr = c[variant]
            assert (arr[ls.MAX_ONLY][:, hit[ls.MAX_ONLY]] == ls.FLT_MAX).all() and np.isnan(arr[ls.NAN_ONLY][:, hit[ls.NAN_ONLY]]).all()
            assert all(np.isnan(res['records'][i, 1]) for i in (ls.MIXED, ls.MAX_ONLY, ls.NAN_ONLY))
            assert all(0 < res['records'][i, 2] <= 1 for i in range(ls.N))                      # a NaN sum next to a finite maximum
            touched, touched2 = ls.sampler_touched(c, r), ls.sampler_touched(c, 2 * r)
            same = sv.same_bits(res['map'], clean['map'])
            assert same[~touched].all() and not same[touched & known].all() and not touched2[ls.CLEAN].any()
            t2 = np.broadcast_to(touched2[:, None], want.shape)
            assert np.isfinite(want[~t2]).all() and np.array_equal(want[~t2], clean_g[~t2])
            assert all(np.isnan(want[i]).any() for i in (ls.MIXED, ls.NAN_ONLY))
            # FLT_MAX: the float32 forward is NaN where the float64 backward is finite
            assert np.isnan(res['map'][ls.MAX_ONLY]).any() and np.isfinite(want[ls.MAX_ONLY]).all()
            if (h, w) == ls.CENSUS_TILE_FRAME:                                                  # the windows straddle the tile edges
                nan_map = np.isnan(res['map'][ls.MIXED])
                assert nan_map[:16, :64].any() and nan_map[:16, 64:].any() and nan_map[16:, :64].any()
        elif variant == 'vectors':
            assert len(c['bad_vec']) == 3 * len(ls.VECTOR_PLANTS)
            for b, y, x in c['bad_vec']:
                assert clean['known'][b, y, x] and not known[b, y, x]
                near = (slice(max(y - r, 0), y + r + 1), slice(max(x - r, 0), x + r + 1))
                lower = known[b][near] & (res['n'][b][near] < clean['n'][b][near])
                assert lower.any(), (b, y, x)                                                   # a known neighbour counts one pixel fewer
            assert np.isfinite(res['records']).all() and np.isfinite(want).all()
        else:
            assert np.isfinite(res['map']).all() and np.isfinite(want).all() and max(share) == 0
            for name in ls.BORDER:
                y, x = c['names'][name][0]
                assert np.all(want[:, :, y, x] != 0), name


def test_ssim_frames_the_issue_rules_out_miss_the_cap_or_come_close():
    """20 x 28 at window 3 and 37 x 53 at window 7 contaminate more than a quarter of the gradient; they are not among the frames"""
    assert (20, 28, 3) not in ls.SSIM_FRAMES and (37, 53, 7) not in ls.SSIM_FRAMES and (37, 53, 5) not in ls.SSIM_FRAMES
    res, (want, big_a) = _ssim(37, 53, 7, 's', 'other')
    assert max(_class_share(want, big_a, res['known'])) > CAP


def _ssim_run(case, window, monkeypatch):
    """(rec, map, loss, gradient) of the product's own autograd route with the oracles in the bindings' place"""
    from oflibpytorch_amd import _ssim
    monkeypatch.setattr(_ssim, "flow_ssim", sso.fake_flow_ssim)
    monkeypatch.setattr(_ssim, "flow_ssim_grad", sso.fake_flow_ssim_grad_for(ls.UPSTREAM))
    sign = ls.sign_of(case['ref'])
    mask, img, other = (torch.from_numpy(np.array(case[k])) for k in ('mask', 'img', 'other'))
    rec, smap = _ssim.flow_ssim(torch.from_numpy(np.array(case['a'])), mask, img, other, sign, window, sso.C1, sso.C2, want_map=True)
    v = torch.from_numpy(np.array(case['a'], np.float32)).requires_grad_(True)
    loss = _ssim.ssim(v, mask, img, other, sign, window, sso.C1, sso.C2)
    assert type(loss.grad_fn).__name__ == "SsimFnBackward"
    loss.backward(torch.tensor(ls.UPSTREAM))
    return rec.numpy(), smap.numpy(), loss.detach().numpy(), v.grad.numpy()


@pytest.mark.parametrize("ref", ls.REFS)
def test_the_ssim_comparison_passes_on_the_oracle_and_fails_on_a_wrong_result(oracle_native, monkeypatch, ref):
    h, w, window = ls.SSIM_FRAMES[0]
    fin_case = ls.ssim_case(h, w, ref, 'finite')
    f_rec, f_map, f_loss, f_grad = _ssim_run(fin_case, window, monkeypatch)
    ls.check_ssim(fin_case, window, f_rec, f_map, f_loss, f_grad, None)
    fin = (f_rec, f_map, f_grad)
    for variant in ('other', 'img', 'vectors'):
        case = ls.ssim_case(h, w, ref, variant)
        rec, smap, loss, grad = _ssim_run(case, window, monkeypatch)
        ratio, share = ls.check_ssim(case, window, rec, smap, loss, grad, fin)
        assert ratio <= 0.5 and share <= CAP                                                   # (the float32 rounding of the oracle's own value)
        known = sso.compute(case['a'], case['mask'], case['img'], case['other'], ref, window)['known']
        by, bx = np.argwhere(known[ls.CLEAN] & np.isfinite(smap[ls.CLEAN]))[5]
        uy, ux = np.argwhere(~known[ls.MIXED])[3]
        one_up, moved, nan_map, nan_grad = smap.copy(), grad.copy(), smap.copy(), grad.copy()
        one_up[ls.CLEAN, by, bx] = np.nextafter(one_up[ls.CLEAN, by, bx], np.float32(2))
        (y0, x0), (y1, x1) = np.argwhere(known[ls.CLEAN])[[7, 8]]
        assert not np.array_equal(grad[ls.CLEAN, :, y0, x0], grad[ls.CLEAN, :, y1, x1])
        moved[ls.CLEAN, :, y0, x0], moved[ls.CLEAN, :, y1, x1] = grad[ls.CLEAN, :, y1, x1], grad[ls.CLEAN, :, y0, x0]
        nan_map[ls.MIXED, uy, ux] = np.nan
        nan_grad[ls.MIXED, 0, uy, ux] = np.nan
        for wrong in ((rec, one_up, loss, grad), (rec, smap, loss, moved), (rec, nan_map, loss, grad), (rec, smap, loss, nan_grad)):
            with pytest.raises(AssertionError):
                ls.check_ssim(case, window, *wrong, fin)


# ---- the cost volume ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cv(h, w, radius, c, ref, variant):
    k = ls.cost_volume_case(h, w, ref, variant, c)
    res = cvo.compute(k['a'], k['mask'], k['feat'], k['other'], ref, radius)
    d_feat, d_w = cvo.grads(k['a'], k['mask'], k['feat'], k['other'], ref, radius, k['g'], res=res)
    return {'volume': res['volume'], 'd_feat': d_feat, 'd_w': d_w, 'warped': res['warped']}


@pytest.mark.parametrize("ref", ls.REFS)
@pytest.mark.parametrize("h,w,radius,c", ls.cv_frames())
def test_cost_volume_cases_meet_their_conditions(h, w, radius, c, ref):
    """Results are held bit for bit, so there is no class cap; instead every image of a special variant keeps at least half of its
    d feat and d W finite, and the mixed and the NaN image hold a non-finite element in the output the variant aims at."""
    assert cvo.geometry() == {"kTileW": 32, "kTileH": 16, "kChanChunk": 16} or c == cvo.geometry()["kChanChunk"] + 1 or radius == 1
    fin = _cv(h, w, radius, c, ref, 'finite')
    f_case = ls.cost_volume_case(h, w, ref, 'finite', c)
    assert all(np.isfinite(fin[k]).all() for k in fin) and 0 <= f_case['feat'].min() and f_case['other'].max() < 1.0
    for variant in ls.CV_VARIANTS[1:]:
        k = ls.cost_volume_case(h, w, ref, variant, c)
        got = _cv(h, w, radius, c, ref, variant)
        bad = {name: [float((~np.isfinite(got[name][i])).mean()) for i in range(ls.N)] for name in ('volume', 'd_feat', 'd_w')}
        print("cost volume %d x %d r %d C %d '%s' %s: not finite: %s" % (h, w, radius, c, ref, variant,
                                                                         {n: np.round(v, 3).tolist() for n, v in bad.items()}))
        assert max(bad['d_feat']) <= 0.5 and max(bad['d_w']) <= 0.5
        assert not any(k[n][ls.CLEAN].any() for n in ('feat_hit', 'other_hit', 'g_hit'))
        aimed = {'other': 'd_feat', 'feat': 'd_w', 'upstream': 'd_w'}.get(variant)
        if aimed:
            assert bad[aimed][ls.MIXED] > 0 and bad[aimed][ls.NAN_ONLY] > 0, variant
            assert bad['volume'][ls.MIXED] > 0 or variant == 'upstream'
        touched = ls.cv_touched(k)
        for name in ('volume', 'd_feat', 'd_w'):
            t = np.broadcast_to(touched[name][:, None], got[name].shape)
            assert np.array_equal(got[name].view(np.uint32)[~t], fin[name].view(np.uint32)[~t]), (variant, name)
            assert t.mean() < 0.6
        if variant in ('other', 'feat'):
            hit = k['other_hit'] if variant == 'other' else k['feat_hit']
            assert hit[ls.MIXED].sum() == (4 if (h, w) == ls.CV_TILE_FRAME else 3)
            arr = k[variant]
            assert (arr[ls.MAX_ONLY][:, hit[ls.MAX_ONLY]] == ls.FLT_MAX).all() and np.isnan(arr[ls.NAN_ONLY][:, hit[ls.NAN_ONLY]]).all()
            if (h, w) == ls.CV_TILE_FRAME:
                assert all(hit[ls.MIXED, y, x] for y, x in ls.CV_TILE_PIXELS)
        if variant == 'other':
            # a weight-0 tap inside the frame turns the sample NaN: the named reader of the weight-0 plant (not at the tile frame)
            if (h, w) != ls.CV_TILE_FRAME:
                y, x = k['names']['weight0_east'][0]
                assert k['usable'][ls.NAN_ONLY, y, x] and np.isnan(got['warped'][ls.NAN_ONLY, :, y, x]).all()
        if variant == 'vectors':
            assert len(k['bad_vec']) == 3 * len(ls.VECTOR_PLANTS)
            assert all(f_case['usable'][b, y, x] and not k['usable'][b, y, x] for b, y, x in k['bad_vec'])
            assert all(np.isfinite(got[n]).all() for n in got)
        if variant == 'unsampled':
            planted = k['other_hit']
            assert planted[:ls.CLEAN].sum((1, 2)).min() >= 2 and not np.isfinite(k['other'][ls.MIXED][:, planted[ls.MIXED]]).all(0).any()
            assert not (ls.readers(k['a'], ref, planted) & k['usable']).any()                   # no usable sample taps them ...
            for b, y, x in np.argwhere(planted):                                               # ... and a pixel that is not usable does
                one = np.zeros_like(planted)
                one[b, y, x] = True
                assert (ls.readers(k['a'], ref, one) & ~k['usable']).any()
            assert all(np.isfinite(got[n]).all() for n in got)
            assert all(np.array_equal(got[n].view(np.uint32), fin[n].view(np.uint32)) for n in got)
        if variant == 'upstream':
            gy, gx = np.nonzero(k['g_hit'][ls.MIXED])
            assert (gy == h - 1).any() and (gx == w - 1).any() and (gy == 15).any() and (gy == 16).any()
            assert w <= 32 or ((gx == 31).any() and (gx == 32).any())
            assert _classes_seen(k['g'][ls.MIXED]) >= {0, 1, 2, 3} and (np.abs(k['g'][ls.MIXED]) == ls.FLT_MAX).any()


def test_cost_volume_at_20_by_28_radius_4_would_lose_more_than_half():
    """The frame the cases avoid: the readers of three planted pixels and a window of 9 x 9 leave under half of d feat finite"""
    fin = ls.sampler_case(20, 28, 's', 'finite', 3, False, True)
    base = ls.sampler_case(20, 28, 's', 'other', 3, False, True)
    other = ls._scaled(base['other'], fin['other'])
    g = cvo.upstream(ls.N, 81, 20, 28)
    d_feat = cvo.grads(fin['a'], fin['mask'], fin['img'] / ls.SCALE, other, 's', 4, g)[0]
    assert max((~np.isfinite(d_feat[i])).mean() for i in range(ls.N)) > 0.5


def _cv_backward(case, monkeypatch):
    """{d feat, d other, d flow} of the product's own CostVolumeFn with the oracles in the bindings' place: d feat and d W from the
    oracle, d other and d flow from its float64 backward of the warp on the chain vectors, rounded to float32"""
    from oflibpytorch_amd import _cost_volume, _native
    for name in ("flow_cost_volume", "flow_cost_volume_grad", "flow_cost_volume_chain", "flow_cost_volume_gate"):
        monkeypatch.setattr(_cost_volume, name, getattr(cvo, "fake_" + name))

    def fake_warp_bwd_grad(flow, src, grad_out, *, flow_sign=1.0, g_scale=1.0, want_src=True, want_flow=True):
        assert np.isfinite(flow.numpy()).all()                                                  # the chain vectors
        with np.errstate(all='ignore'):
            d_other, d_flow = cvo.chain(flow.numpy(), src.numpy(), grad_out.numpy(), 's' if flow_sign < 0 else 't')
            return torch.from_numpy(d_other.astype(np.float32)), torch.from_numpy(d_flow.astype(np.float32))
    monkeypatch.setattr(_native, "warp_bwd_grad", fake_warp_bwd_grad)
    v, ft, ot = (torch.from_numpy(np.array(case[k], np.float32)).requires_grad_(True) for k in ('a', 'feat', 'other'))
    vol = _cost_volume.cost_volume(v, torch.from_numpy(np.array(case['mask'])), ft, ot, ls.sign_of(case['ref']), case['radius'])
    assert type(vol.grad_fn).__name__ == "CostVolumeFnBackward"
    vol.backward(torch.from_numpy(np.array(case['g'])))
    return {'d_feat': ft.grad.numpy(), 'd_other': ot.grad.numpy(), 'd_flow': v.grad.numpy()}


@pytest.mark.parametrize("ref", ls.REFS)
def test_the_cost_volume_comparisons_pass_on_the_oracle_and_fail_on_a_wrong_result(oracle_native, monkeypatch, ref):
    h, w, radius, c = ls.cv_frames()[0]
    fin = {k: v for k, v in _cv(h, w, radius, c, ref, 'finite').items() if k != 'warped'}
    f_case = ls.cost_volume_case(h, w, ref, 'finite', c)
    ls.check_cost_volume_kernels(f_case, fin, None)
    fin_b = _cv_backward(f_case, monkeypatch)
    ls.check_cost_volume_backward(f_case, fin_b, None)
    for variant in ls.CV_VARIANTS[1:]:
        case = ls.cost_volume_case(h, w, ref, variant, c)
        got = {k: v for k, v in _cv(h, w, radius, c, ref, variant).items() if k != 'warped'}
        ls.check_cost_volume_kernels(case, got, fin)
        back = _cv_backward(case, monkeypatch)
        ls.check_cost_volume_backward(case, back, fin_b)
        usable = case['usable']
        py, px = np.argwhere(usable[ls.CLEAN])[9]
        (y0, x0), (y1, x1) = np.argwhere(usable[ls.CLEAN])[[11, 12]]
        uy, ux = np.argwhere(~usable[ls.MIXED])[2]
        one_up = dict(got, volume=got['volume'].copy())
        v = one_up['volume'][ls.CLEAN, 4, py, px]
        assert np.isfinite(v) and v != 0
        one_up['volume'][ls.CLEAN, 4, py, px] = np.nextafter(v, np.float32(np.inf))
        moved = dict(got, d_feat=got['d_feat'].copy())
        moved['d_feat'][ls.CLEAN, :, y0, x0], moved['d_feat'][ls.CLEAN, :, y1, x1] = got['d_feat'][ls.CLEAN, :, y1, x1], got['d_feat'][ls.CLEAN, :, y0, x0]
        assert not np.array_equal(moved['d_feat'], got['d_feat'])
        nan_w = dict(got, d_w=got['d_w'].copy())
        nan_w['d_w'][ls.MIXED, 0, uy, ux] = np.nan
        for wrong in (one_up, moved, nan_w):
            with pytest.raises(AssertionError):
                ls.check_cost_volume_kernels(case, wrong, fin)
        nan_flow = dict(back, d_flow=back['d_flow'].copy())
        nan_flow['d_flow'][ls.MIXED, 1, uy, ux] = np.nan
        up_other = dict(back, d_other=back['d_other'].copy())
        up_other['d_other'][ls.CLEAN, 0, py, px] += np.float32(0.01) * np.abs(back['d_other']).max() + np.float32(1e-3)
        moved_flow = dict(back, d_flow=back['d_flow'].copy())
        moved_flow['d_flow'][ls.CLEAN, :, y0, x0], moved_flow['d_flow'][ls.CLEAN, :, y1, x1] = back['d_flow'][ls.CLEAN, :, y1, x1], back['d_flow'][ls.CLEAN, :, y0, x0]
        assert not np.array_equal(moved_flow['d_flow'], back['d_flow'])
        for wrong in (nan_flow, up_other, moved_flow):
            with pytest.raises(AssertionError):
                ls.check_cost_volume_backward(case, wrong, fin_b)


def test_the_chain_vectors_and_the_gate_of_the_cost_volume_backward():
    """What `CostVolumeFn.backward` hands the backward of the warp: the flow's own vectors bit for bit where they are finite, a vector
    that leaves no tap inside the frame where they are not; without the two, the float64 backward of the warp gives NaN on 'unsampled'
    and 'vectors' at pixels that are not usable."""
    h, w, radius, c = ls.cv_frames()[0]
    for ref in ls.REFS:
        case = ls.cost_volume_case(h, w, ref, 'vectors', c)
        chain = cvo.chain_vectors(case['a'], ref)
        bad = ~np.isfinite(case['a']).all(1)
        assert bad.sum() == len(case['bad_vec']) and np.isfinite(chain).all()
        assert np.array_equal(chain.view(np.uint32)[~np.broadcast_to(bad[:, None], chain.shape)],
                              np.asarray(case['a']).view(np.uint32)[~np.broadcast_to(bad[:, None], chain.shape)])
        t = go.warp_taps(chain, ls.N, ls.sign_of(ref))
        assert not any(t.ok[j][bad].any() for j in range(4))
        case = ls.cost_volume_case(h, w, ref, 'unsampled', c)
        d_w = cvo.grads(case['a'], case['mask'], case['feat'], case['other'], ref, radius, case['g'])[1]
        with np.errstate(all='ignore'):
            d_flow = cvo.chain(case['a'], case['other'], d_w, ref)[1]
        nan_at = np.isnan(d_flow).any(1)
        assert nan_at[:ls.CLEAN].any() and not (nan_at & case['usable']).any()                  # 0 * tap at pixels that are not usable


# ---- the two oracles return the bits they returned before these cases existed -------------------------------------------------------
def test_the_ssim_and_cost_volume_oracles_keep_their_bits_on_finite_input():
    import hashlib
    import photometric_oracle as po

    def digest(*arrays):
        m = hashlib.sha256()
        for x in arrays:
            m.update(np.ascontiguousarray(x).tobytes())
        return m.hexdigest()[:16]
    a, m, img, other, _, _ = po.case(2, 20, 28, 's')
    res = sso.compute(a, m, img, other, 's', 3)
    want, big_a = sso.grad(a, m, img, other, 's', 3, res=res)
    assert digest(res['map'], res['records'], want, big_a) == SSIM_DIGEST
    a, m = cvo.case(2, 20, 28, 't')
    feat, oth = cvo.features(2, 3, 20, 28, 't')
    g = cvo.upstream(2, 25, 20, 28)
    r2 = cvo.compute(a, m, feat, oth, 't', 2)
    assert digest(r2['volume'], *cvo.grads(a, m, feat, oth, 't', 2, g, res=r2)) == CV_DIGEST


SSIM_DIGEST = "299645191dcd59e5"
CV_DIGEST = "a55ab3c0595e2e8d"
