"""Non-finite values through the global matching on the device (ofl_matching.hip): everything is IEEE as the steps give
it.  A NaN in feat(p) makes the flow and prob of p NaN, d feat(p) NaN in every channel and d other NaN wherever p contributes, which is
every position; a NaN in other(q) makes every pixel NaN, because the softmax sees every q; a +-inf feature that drives a logit to +inf
gives NaN (inf - inf), one that drives it to -inf a weight of exactly 0.  Every element outside the special's reach carries the bits of
the run without the special (device against device: no bar is involved).  Flow.from_matching on such input raises the constructor's
ordinary error for non-finite vectors, so these tests call `_matching` directly."""
import numpy as np
import pytest
import torch

import matching_oracle as mo

pytestmark = pytest.mark.gpu

N, C, H, W = 2, 3, 5, 7                              # Q = 35: two chunks
IMG = 1                                              # the image that gets the special; the other stays clean


def _to(x):
    return torch.from_numpy(np.ascontiguousarray(x).copy()).to(torch.device('cuda', 0))


def _run(feat, other, g, sign=-1.0):
    from oflibpytorch_amd import _matching
    ft, ot = _to(feat), _to(other)
    out, prob, stats = _matching.flow_global_match(ft, ot, sign, True, True)
    df, do = _matching.flow_global_match_grad(ft, ot, sign, stats, _to(g))
    return out.cpu().numpy(), prob.cpu().numpy(), df.cpu().numpy(), do.cpu().numpy()


def _check(name, got, clean, bad):
    """Exactly `bad` is NaN; everything else has the clean run's bits"""
    assert bad.shape == got.shape and bad.any()
    assert np.array_equal(np.isnan(got), bad), "%s: %d NaN elements, %d expected" % (name, np.isnan(got).sum(), bad.sum())
    assert np.array_equal(got.view(np.uint32)[~bad], clean.view(np.uint32)[~bad]), name + ": an element outside the special's reach changed"


def _inputs():
    feat, other = (a.copy() for a in mo.features_general(N, C, H, W))
    return feat, other, mo.upstream(N, H, W)


@pytest.mark.parametrize("y,x", [(2, 3), (0, 0), (H - 1, W - 1)])
def test_a_nan_in_feat_reaches_its_pixel_and_every_position(y, x):
    feat, other, g = _inputs()
    clean = _run(feat, other, g)
    assert all(np.isfinite(a).all() for a in clean)
    feat[IMG, 1, y, x] = np.nan
    out, prob, df, do = _run(feat, other, g)
    bad = np.zeros((N, 2, H, W), bool)
    bad[IMG, :, y, x] = True
    _check("forward", out, clean[0], bad)
    _check("prob", prob, clean[1], bad[:, 0])
    bad = np.zeros((N, C, H, W), bool)
    bad[IMG, :, y, x] = True
    _check("d feat", df, clean[2], bad)
    bad = np.zeros((N, C, H, W), bool)
    bad[IMG] = True
    _check("d other", do, clean[3], bad)


@pytest.mark.parametrize("y,x", [(2, 3), (0, 0), (H - 1, W - 1)])
def test_a_nan_in_other_reaches_every_pixel(y, x):
    feat, other, g = _inputs()
    clean = _run(feat, other, g)
    other[IMG, 2, y, x] = np.nan
    res = _run(feat, other, g)
    for name, got, ref in zip(("forward", "prob", "d feat", "d other"), res, clean):
        bad = np.zeros(got.shape, bool)
        bad[IMG] = True
        _check(name, got, ref, bad)


@pytest.mark.parametrize("value", [np.inf, -np.inf])
def test_an_infinite_feature_gives_nan_at_plus_inf_and_a_weight_of_zero_at_minus_inf(value):
    """other_0(q) = +-inf at q = (2, 1): the logit of p is +inf where value * feat_0(p) > 0 (inf - inf: NaN), NaN where feat_0(p) = 0
    (0 * inf) and -inf where it is < 0: a weight of exactly 0, so the pixel stays finite and its flow is the oracle's, which takes the same
    IEEE steps.  The image without the special keeps its bits."""
    feat, other, g = _inputs()
    clean = _run(feat, other, g)
    other[IMG, 0, 2, 1] = value
    out, prob, df, do = _run(feat, other, g)
    for got, ref in zip((out, prob, df, do), clean):
        assert np.array_equal(got[1 - IMG].view(np.uint32), ref[1 - IMG].view(np.uint32))
    zero = feat[IMG, 0] * np.float32(np.sign(value)) < 0                                     # the pixels whose logit at q is -inf
    assert zero.any() and (~zero).any()
    assert np.isnan(out[IMG][:, ~zero]).all() and np.isnan(prob[IMG][~zero]).all()
    assert np.isfinite(out[IMG][:, zero]).all() and np.isfinite(prob[IMG][zero]).all()
    with np.errstate(all='ignore'):
        want = mo.compute(feat, other, -1.0)
        gr = mo.grads(feat, other, -1.0, g)
    q = H * W
    assert (want['w'][IMG].reshape(H, W, q)[zero][:, 2 * W + 1] == 0).all()                  # exactly 0
    bar = mo.ulp32(want['out'][IMG][:, zero]) + 2.0 ** -mo.forward_shift(q) * want['mag'][IMG][:, zero]
    assert (np.abs(out[IMG][:, zero] - want['out'][IMG][:, zero]) <= bar).all()
    # the gradients are NaN exactly where the oracle's are (0 * inf in channel 0 of d feat; every p reaches every q in d other)
    assert np.array_equal(np.isnan(df), np.isnan(gr['d_feat'])) and np.array_equal(np.isnan(do), np.isnan(gr['d_other']))
    fin = np.isfinite(gr['d_feat64'])
    assert fin[IMG].any()
    bar = mo.ulp32(gr['d_feat64'][fin]) + 2.0 ** -mo.grad_shift(q) * gr['mag_feat'][fin]
    assert (np.abs(df[fin] - gr['d_feat64'][fin]) <= bar).all()


def test_the_api_raises_the_constructors_error():
    import oflibpytorch_amd as ofl
    feat, other, _ = _inputs()
    feat[IMG, 1, 2, 3] = np.nan
    with pytest.raises(ValueError, match="Error setting flow vectors"):
        ofl.Flow.from_matching(_to(feat), _to(other), 's')
