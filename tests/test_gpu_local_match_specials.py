"""Non-finite values through Flow.match_local (ofl_local_match.hip): each case plants one special value and compares every
other element with the bits of the run without it.  9 x 17 (both extents minus one are powers of two: an integer vector samples a value
of `other` bit for bit), C = 3, both references; the bindings and `_autograd.LocalMatchFn` are called directly where the flow's
constructor would refuse the vectors."""
import numpy as np
import pytest
import torch

import local_match_oracle as lo

pytestmark = pytest.mark.gpu
N, C, H, W = 1, 3, 9, 17


def _dev():
    return torch.device('cuda', 0)


def _to(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x).copy()).to(_dev())


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _forward(a, mask, feat, other, ref, radius):
    from oflibpytorch_amd import _local_match
    out, prob, stats = _local_match.flow_local_match(_to(a), _to(mask), _to(feat), _to(other), lo.sign_of(ref), radius, True, True)
    return out.cpu().numpy(), prob.cpu().numpy(), stats


def _grads(a, mask, feat, other, ref, radius, stats, g):
    from oflibpytorch_amd import _local_match
    df, dw = _local_match.flow_local_match_grad(_to(a), _to(mask), _to(feat), _to(other), lo.sign_of(ref), radius, stats, _to(g))
    return df.cpu().numpy(), dw.cpu().numpy()


def _backward(a, mask, feat, other, ref, radius, g):
    """(out, d flow, d feat, d other) of the autograd route"""
    from oflibpytorch_amd import _autograd
    at, ft, ot = (_to(x).requires_grad_(True) for x in (a, feat, other))
    out, _ = _autograd.LocalMatchFn.apply(at, _to(mask), ft, ot, lo.sign_of(ref), radius, False)
    out.backward(_to(g))
    return tuple(t.cpu().numpy() for t in (out.detach(), at.grad, ft.grad, ot.grad))


def _near(y, x, radius):
    """bool [H, W]: the pixels within `radius` of (y, x)"""
    yy, xx = np.mgrid[0:H, 0:W]
    return (np.abs(yy - y) <= radius) & (np.abs(xx - x) <= radius)


def _same_elsewhere(got, clean, where, what):
    """`got` equals `clean` bit for bit outside `where` ([H, W], broadcast over the leading axes)"""
    keep = ~np.broadcast_to(where, got.shape)
    assert np.array_equal(_bits(got)[keep], _bits(clean)[keep]), what


def _inputs():
    feat, other = (x.copy() for x in lo.features_general(N, C, H, W))
    return lo.vectors_general(N, H, W).copy(), lo.masks(N, H, W)['checker'], feat, other, lo.upstream(N, H, W)


@pytest.mark.parametrize("ref", lo.REFS)
@pytest.mark.parametrize("radius", [1, 4])
def test_a_nan_in_feat_stays_at_its_pixel(radius, ref):
    a, mask, feat, other, g = _inputs()
    out0, prob0, stats0 = _forward(a, mask, feat, other, ref, radius)
    df0, _ = _grads(a, mask, feat, other, ref, radius, stats0, g)
    y, x = 4, 8
    feat[0, 1, y, x] = np.nan
    out1, prob1, stats1 = _forward(a, mask, feat, other, ref, radius)
    df1, _ = _grads(a, mask, feat, other, ref, radius, stats1, g)
    here = _near(y, x, 0)
    assert np.isnan(out1[0, :, y, x]).all() and np.isnan(prob1[0, y, x]) and np.isnan(df1[0, :, y, x]).all()
    assert np.isfinite(out0).all() and np.isfinite(df0).all()
    _same_elsewhere(out1, out0, here, "forward")
    _same_elsewhere(prob1, prob0, here, "prob")
    _same_elsewhere(df1, df0, here, "d feat")


@pytest.mark.parametrize("ref", lo.REFS)
@pytest.mark.parametrize("radius", [1, 3])
def test_a_nan_in_other_reaches_the_windows_that_hold_its_samplers(radius, ref):
    """Exactly the pixels within r of a pixel whose W' the oracle finds NaN -- a usable pixel with the NaN among its four taps, whatever
    the tap's weight -- are NaN; every other pixel keeps its bits"""
    a, mask, feat, other, _ = _inputs()
    out0, prob0, _ = _forward(a, mask, feat, other, ref, radius)
    other[0, 0, 4, 8] = np.nan
    out1, prob1, _ = _forward(a, mask, feat, other, ref, radius)
    wp, usable, _ = lo.warped(a, mask, other, ref)
    hit = np.isnan(wp[0]).any(0)
    assert hit.any() and (hit & usable[0]).sum() == hit.sum()
    want = np.zeros((H, W), bool)
    for y, x in zip(*np.nonzero(hit)):
        want |= _near(y, x, radius)
    assert not want.all()
    assert np.array_equal(np.isnan(out1[0]).all(0), want) and np.array_equal(np.isnan(out1[0]).any(0), want)
    assert np.array_equal(np.isnan(prob1[0]), want)
    _same_elsewhere(out1, out0, want, "forward")
    _same_elsewhere(prob1, prob0, want, "prob")


@pytest.mark.parametrize("ref", lo.REFS)
def test_non_finite_values_of_other_that_only_unusable_pixels_sample_change_no_bit(ref):
    """Every vector shifts by three columns, so that no usable pixel samples the first three columns of `other`; one pixel that the mask
    excludes points into them, at a NaN with +inf and -inf beside it"""
    radius = 2
    _, _, feat, other, g = _inputs()
    sign = lo.sign_of(ref)
    a = np.zeros((N, 2, H, W), np.float32)
    a[:, 0] = 3.0 * -sign
    a[0, 0, 4, 5] = -4.0 * -sign                                                             # samples (1, 4) with the taps (2, 4), (1, 5), (2, 5)
    mask = np.ones((N, H, W), bool)
    mask[0, 4, 5] = False
    clean = _backward(a, mask, feat, other, ref, radius, g)
    other[0, :, 4, 1], other[0, :, 4, 2], other[0, :, 5, 1] = np.nan, np.inf, -np.inf
    usable = lo.usable_of(a, mask, ref)
    assert not usable[0, 4, 5] and usable[0, :, :W - 4].sum() == H * (W - 4) - 1
    dirty = _backward(a, mask, feat, other, ref, radius, g)
    for name, x, y in zip(("forward", "d flow", "d feat", "d other"), dirty, clean):
        assert np.isfinite(y).all(), name
        assert np.array_equal(_bits(x), _bits(y)), name
    assert np.array_equal(_bits(dirty[1][0, :, 4, 5]), _bits(g[0, :, 4, 5]))                 # d flow is g itself where the pixel is not usable


@pytest.mark.parametrize("ref", lo.REFS)
def test_infinite_logits(ref):
    """A zero flow, positive features: W' = -inf at one pixel puts the logit -inf into every window that holds it, whose weight is exactly
    0 -- the vectors stay finite, within the bar of the general tier, d W there is exactly 0 and d feat of those windows, whose term
    0 * -inf is formed, NaN -- and W' = +inf makes those windows NaN
    and no other.  The three neighbours that have the pixel among their zero-weight taps are masked out, so that they load no sample."""
    radius = 2
    _, _, feat, other, g = _inputs()
    feat = (np.abs(feat) + np.float32(2.0 ** -6)).astype(np.float32)
    a = np.zeros((N, 2, H, W), np.float32)
    y, x = 4, 8
    mask = np.ones((N, H, W), bool)
    mask[0, y, x - 1] = mask[0, y - 1, x] = mask[0, y - 1, x - 1] = False
    out0, prob0, _ = _forward(a, mask, feat, other, ref, radius)
    near = _near(y, x, radius)
    other[0, :, y, x] = -np.inf
    out1, prob1, stats1 = _forward(a, mask, feat, other, ref, radius)
    df1, dw1 = _grads(a, mask, feat, other, ref, radius, stats1, g)
    fwd = lo.compute(a, mask, feat, other, ref, radius)
    assert np.isneginf(fwd['warped'][0, :, y, x]).all() and np.isfinite(np.delete(fwd['warped'].reshape(C, -1), y * W + x, 1)).all()
    assert (fwd['w'][0][np.isneginf(fwd['s'][0])] == 0).all() and np.isneginf(fwd['s'][0]).sum() == near.sum()
    assert np.isfinite(out1).all() and np.isfinite(prob1).all()
    assert np.array_equal(np.isnan(df1[0]).all(0), near) and np.array_equal(np.isnan(df1[0]).any(0), near)   # (0 * -inf: the product is formed)
    bar = lo.ulp32(fwd['out']) + 2.0 ** -lo.forward_shift(fwd['terms'])[:, None].astype(np.float64) * fwd['mag']
    assert (np.abs(out1 - fwd['out']) <= bar).all()
    assert (dw1[0, :, y, x] == 0).all()
    _same_elsewhere(out1, out0, near, "forward under -inf")
    other[0, :, y, x] = np.inf
    out2, prob2, _ = _forward(a, mask, feat, other, ref, radius)
    assert np.array_equal(np.isnan(out2[0]).all(0), near) and np.array_equal(np.isnan(prob2[0]), near)
    _same_elsewhere(out2, out0, near, "forward under +inf")


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("ref", lo.REFS)
def test_a_non_finite_vector_component_makes_its_pixel_unusable(ref, bad):
    """The pixel enters every window with W' = +0, as if the mask excluded it: every other vector, d feat and d other carry the bits of
    that run, and d flow at the pixel is g"""
    radius = 2
    a, mask, feat, other, g = _inputs()
    y, x = 4, 8
    mask[0, y, x] = True
    a[0, :, y, x] = (0.5, -0.25)
    assert lo.usable_of(a, mask, ref)[0, y, x]
    masked = mask.copy()
    masked[0, y, x] = False
    clean = _backward(a, masked, feat, other, ref, radius, g)
    a[0, 1, y, x] = bad
    dirty = _backward(a, mask, feat, other, ref, radius, g)
    here = _near(y, x, 0)
    for name, p, q in zip(("forward", "d flow", "d feat", "d other"), dirty, clean):
        assert np.isfinite(q).all(), name
        if name == "d other":
            assert np.array_equal(_bits(p), _bits(q)), name
        else:
            _same_elsewhere(p, q, here, name)
    assert not np.isfinite(dirty[0][0, 1, y, x]) and dirty[0][0, 0, y, x] == clean[0][0, 0, y, x]
    assert np.array_equal(_bits(dirty[1][0, :, y, x]), _bits(g[0, :, y, x]))                 # d flow there is g
    assert np.array_equal(_bits(dirty[2]), _bits(clean[2]))                                  # d feat: every pixel
