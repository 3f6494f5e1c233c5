"""Non-finite values through the flow propagation on the device (ofl_propagate.hip): everything is IEEE as the steps give
it.  A NaN in query(p) makes the result of p and d query(p) NaN, and of the forward and d query nothing else; d key and d flow are NaN
wherever p contributes.  A NaN in key(q) makes every pixel of its image NaN in the global form and exactly the pixels within r in the
local form.  A NaN in the key and the vector of an EXCLUDED position changes no bit of the forward -- it contributes no step -- and makes
the gradients NaN exactly where the definition forms 0 * NaN.  A +-inf key that drives a logit to +inf gives NaN (inf - inf), one that
drives it to -inf a weight of exactly 0.  The gradients are NaN exactly where the oracle's are, and every element outside the special's
reach carries the bits of the run without the special (device against device: no bar is involved).  Flow's constructor rejects non-finite
vectors, so these tests call `_propagate` directly."""
import numpy as np
import pytest
import torch

import propagate_oracle as po

pytestmark = pytest.mark.gpu

N, C, H, W = 2, 3, 5, 7                              # Q = 35: two chunks; wider and higher than the window of radius 2
IMG = 1                                              # the image that gets the special; the other stays clean
FORMS = [None, 2]
NAMES = ("forward", "d query", "d key", "d flow")


def _to(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x).copy()).to(torch.device('cuda', 0))


def _run(flow, mask, query, key, g, radius):
    from oflibpytorch_amd import _propagate
    ft, mt, qt, kt = _to(flow), _to(mask), _to(query), _to(key)
    out, _, stats = _propagate.flow_propagate(ft, mt, qt, kt, radius, True)
    grads = _propagate.flow_propagate_grad(ft, mt, qt, kt, radius, stats, _to(g))
    return (out.cpu().numpy(),) + tuple(d.cpu().numpy() for d in grads)


def _oracle(flow, mask, query, key, g, radius):
    with np.errstate(all='ignore'):
        fw, gr = po.compute(flow, mask, query, key, radius), po.grads(flow, mask, query, key, radius, g)
    return fw['out32'], gr['d_query'], gr['d_key'], gr['d_flow']


def _check(name, got, clean, bad):
    """Exactly `bad` is NaN; everything else has the clean run's bits"""
    assert bad.shape == got.shape
    assert np.array_equal(np.isnan(got), bad), "%s: %d NaN elements, %d expected" % (name, np.isnan(got).sum(), bad.sum())
    assert np.array_equal(got.view(np.uint32)[~bad], clean.view(np.uint32)[~bad]), name + ": an element outside the special's reach changed"


def _inputs():
    query, key = (a.copy() for a in po.features_general(N, C, H, W))
    return po.vectors(N, H, W).copy(), query, key, po.upstream(N, H, W)


def _near(y, x, radius):
    """The pixels whose window holds (y, x): all of them in the global form"""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.ones((H, W), bool) if radius is None else (np.abs(yy - y) <= radius) & (np.abs(xx - x) <= radius)


@pytest.mark.parametrize("radius", FORMS)
@pytest.mark.parametrize("y,x", [(2, 3), (0, 0), (H - 1, W - 1)])
def test_a_nan_in_query_reaches_its_own_pixel(y, x, radius):
    flow, query, key, g = _inputs()
    clean = _run(flow, None, query, key, g, radius)
    assert all(np.isfinite(a).all() for a in clean)
    query[IMG, 1, y, x] = np.nan
    res = _run(flow, None, query, key, g, radius)
    want = _oracle(flow, None, query, key, g, radius)
    bad = np.zeros((N, 2, H, W), bool)
    bad[IMG, :, y, x] = True
    _check("forward", res[0], clean[0], bad)
    bad = np.zeros((N, C, H, W), bool)
    bad[IMG, :, y, x] = True
    _check("d query", res[1], clean[1], bad)
    # d key and d flow: wherever p contributes -- every position of the image, or those of its window
    reach = np.zeros((N, H, W), bool)
    reach[IMG] = _near(y, x, radius)
    _check("d key", res[2], clean[2], np.broadcast_to(reach[:, None], (N, C, H, W)))
    _check("d flow", res[3], clean[3], np.broadcast_to(reach[:, None], (N, 2, H, W)))
    for name, got, exp in zip(NAMES, res, want):
        assert np.array_equal(np.isnan(got), np.isnan(exp)), name


@pytest.mark.parametrize("radius", FORMS)
@pytest.mark.parametrize("y,x", [(2, 3), (0, 0), (H - 1, W - 1)])
def test_a_nan_in_key_reaches_every_pixel_that_sees_it(y, x, radius):
    flow, query, key, g = _inputs()
    clean = _run(flow, None, query, key, g, radius)
    key[IMG, 2, y, x] = np.nan
    res = _run(flow, None, query, key, g, radius)
    want = _oracle(flow, None, query, key, g, radius)
    reach = np.zeros((N, H, W), bool)
    reach[IMG] = _near(y, x, radius)
    _check("forward", res[0], clean[0], np.broadcast_to(reach[:, None], (N, 2, H, W)))
    _check("d query", res[1], clean[1], np.broadcast_to(reach[:, None], (N, C, H, W)))
    for name, got, exp, ref in zip(NAMES, res, want, clean):
        _check(name, got, ref, np.isnan(exp))
    # a pixel that sees the NaN gives a NaN dss to every position of its window: d key and d flow are NaN that far again
    wide = np.zeros((N, H, W), bool)
    wide[IMG] = True if radius is None else _near(y, x, 2 * radius)
    assert np.array_equal(np.isnan(res[3]), np.broadcast_to(wide[:, None], (N, 2, H, W)))


@pytest.mark.parametrize("radius", FORMS)
@pytest.mark.parametrize("y,x", [(2, 3), (0, 0), (H - 1, W - 1)])
def test_a_nan_at_an_excluded_position_leaves_the_forward_alone(y, x, radius):
    flow, query, key, g = _inputs()
    mask = np.ones((N, H, W), bool)
    mask[IMG, y, x] = False
    mask[:, 1, 1] = False                                                                    # (and an excluded position without a special)
    clean = _run(flow, mask, query, key, g, radius)
    assert all(np.isfinite(a).all() for a in clean)
    key[IMG, 2, y, x] = np.nan
    flow[IMG, :, y, x] = np.nan
    res = _run(flow, mask, query, key, g, radius)
    want = _oracle(flow, mask, query, key, g, radius)
    assert np.array_equal(res[0].view(np.uint32), clean[0].view(np.uint32)), "forward: an excluded position changed a bit"
    # d query_c(p) = ... + (+0) * key_c(q): NaN in the channel of the NaN, for every pixel that sees q; d key and d flow hold no NaN
    bad = np.zeros((N, C, H, W), bool)
    bad[IMG, 2] = _near(y, x, radius)
    _check("d query", res[1], clean[1], bad)
    _check("d key", res[2], clean[2], np.zeros((N, C, H, W), bool))
    _check("d flow", res[3], clean[3], np.zeros((N, 2, H, W), bool))
    for name, got, exp in zip(NAMES, res, want):
        assert np.array_equal(np.isnan(got), np.isnan(exp)), name


@pytest.mark.parametrize("radius", FORMS)
@pytest.mark.parametrize("value", [np.inf, -np.inf])
def test_an_infinite_key_gives_nan_at_plus_inf_and_a_weight_of_zero_at_minus_inf(value, radius):
    """key_0(q) = +-inf at q = (2, 1): the logit of a pixel p that sees q is +inf where value * query_0(p) > 0 (inf - inf: NaN), NaN where
    query_0(p) = 0 (0 * inf) and -inf where it is < 0: a weight of exactly 0, so the pixel stays finite and its result is the oracle's,
    which takes the same IEEE steps.  The image without the special, and the pixels that do not see q, keep their bits."""
    flow, query, key, g = _inputs()
    clean = _run(flow, None, query, key, g, radius)
    key[IMG, 0, 2, 1] = value
    res = _run(flow, None, query, key, g, radius)
    sees = _near(2, 1, radius)
    for got, ref in zip(res, clean):
        assert np.array_equal(got[1 - IMG].view(np.uint32), ref[1 - IMG].view(np.uint32))
    assert np.array_equal(res[0][IMG][:, ~sees].view(np.uint32), clean[0][IMG][:, ~sees].view(np.uint32))
    assert np.array_equal(res[1][IMG][:, ~sees].view(np.uint32), clean[1][IMG][:, ~sees].view(np.uint32))
    zero = (query[IMG, 0] * np.float32(np.sign(value)) < 0) & sees                          # the pixels whose logit at q is -inf
    rest = sees & ~zero
    assert zero.any() and rest.any()
    out = res[0]
    assert np.isnan(out[IMG][:, rest]).all() and np.isfinite(out[IMG][:, zero]).all()
    with np.errstate(all='ignore'):
        fw = po.compute(flow, None, query, key, radius)
        gr = po.grads(flow, None, query, key, radius, g)
    step = np.nonzero(fw['idx'].reshape(H, W, -1)[zero] == 2 * W + 1)
    assert len(step[0]) == int(zero.sum()) and (fw['w'][IMG].reshape(H, W, -1)[zero][step] == 0).all()        # exactly 0
    shift = po.forward_shift(fw['terms'])[:, None]
    bar = po.ulp32(fw['out']) + 2.0 ** -shift.astype(np.float64) * fw['mag']
    ok = np.broadcast_to(zero[None], (2, H, W))
    assert (np.abs(out[IMG] - fw['out'][IMG])[ok] <= bar[IMG][ok]).all()
    # the gradients are NaN exactly where the oracle's are, and within their bars where they are finite
    for got, name in zip(res[1:], ('d_query', 'd_key', 'd_flow')):
        assert np.array_equal(np.isnan(got), np.isnan(gr[name])), name
        fin = np.isfinite(gr[name + '64'])
        assert fin[IMG].any() or (name != 'd_query' and radius is None)                    # (global: a NaN pixel reaches every d key, d flow)
        bar = po.ulp32(gr[name + '64'][fin]) + 2.0 ** -po.grad_shift(gr['terms_' + name][fin]).astype(np.float64) * gr['mag_' + name][fin]
        assert (np.abs(got[fin] - gr[name + '64'][fin]) <= bar).all(), name


def test_the_api_raises_the_constructors_error_for_a_non_finite_flow():
    import oflibpytorch_amd as ofl
    flow, query, key, _ = _inputs()
    flow[IMG, 0, 2, 3] = np.nan
    with pytest.raises(ValueError, match="Error setting flow vectors"):
        ofl.Flow(_to(flow), 't').propagate(_to(query), _to(key))
