"""Non-finite and subnormal values through the global matching of fp16 / bf16 features on the device (ofl_matching_x16.hip; DESIGN.md
3.32, "Values that are not finite" and "Subnormal inputs").  The sets of 3.27 hold per pixel and image: a NaN in feat(p) makes the flow
and prob of p NaN, d feat(p) NaN in every channel and d other NaN at every position of the image; a NaN in other(q) makes every pixel of
the image NaN; a +-inf feature that drives a logit to +inf gives NaN, to NaN (0 * inf in a REAL channel) NaN, to -inf a weight of exactly
0 and a finite pixel.  The specials stand at the first pixel, the last one -- the last valid position before the padded tail of the
last chunk -- and inside the frame.  Where this route differs from 3.27: a logit of -inf has the weight 0 at the first position as well
(there the float32 route's chain starts on m = -inf and gives NaN).  The padded channels (C = 3 of 16) multiply zero with zero and add
nothing that is not finite.  Every element outside the special's reach carries the bits of the run without the special (device against
device: no bar is involved).

Subnormal inputs: the MFMA takes fp16 and bf16 subnormals at their value, it does not flush them.  Measured and pinned at one named
input each: C = 1, feat = 1023 * 2^-24 (the largest fp16 subnormal) at every pixel against other = 65504 at the last position and 0
elsewhere -- a logit of 3.994 if the subnormal counts and of 0 if it is flushed, a flow towards the last position or towards the
centroid --, and feat = 127 * 2^-133 against other = 2^127 in bf16 (a logit of 1.98)."""
import numpy as np
import pytest
import torch

import matching_oracle as mo
import matching_x16_oracle as xo

pytestmark = pytest.mark.gpu

N, C, H, W = 2, 3, 5, 7                              # Q = 35: one tile, a chunk and a tail of 3 positions; 13 padded channels
IMG = 1                                              # the image that gets the special; the other stays clean
PLACES = [(2, 3), (0, 0), (H - 1, W - 1)]
NAMES = ('fp16', 'bf16')


def _dev():
    return torch.device('cuda', 0)


def _run(feat, other, g, name, sign=-1.0):
    """(out, prob float32; d feat, d other as float32 views of the dtype's values): the forward, and the float32 gradient kernels on its
    statistics, rounded once -- what the autograd function does"""
    from oflibpytorch_amd import _matching
    dtype = xo.DTYPES[name]
    ft, ot = (torch.from_numpy(np.ascontiguousarray(a).copy()).to(dtype).to(_dev()) for a in (feat, other))
    out, prob, stats = _matching.flow_global_match_x16(ft, ot, sign, True, True)
    df, do = _matching.flow_global_match_grad(ft.float(), ot.float(), sign, stats, torch.from_numpy(g.copy()).to(_dev()))
    return out.cpu().numpy(), prob.cpu().numpy(), df.to(dtype).float().cpu().numpy(), do.to(dtype).float().cpu().numpy()


def _check(what, got, clean, bad):
    """Exactly `bad` is NaN; everything else has the clean run's bits"""
    assert bad.shape == got.shape and bad.any()
    assert np.array_equal(np.isnan(got), bad), "%s: %d NaN elements, %d expected" % (what, np.isnan(got).sum(), bad.sum())
    assert np.array_equal(got.view(np.uint32)[~bad], clean.view(np.uint32)[~bad]), what + ": an element outside the special's reach changed"


def _inputs(name):
    _, _, fup, oup = xo.features_general(name, N, C, H, W)
    return fup.copy(), oup.copy(), mo.upstream(N, H, W)


def test_a_nan_in_feat_reaches_its_pixel_and_every_position():
    for name in NAMES:
        for y, x in PLACES:
            _nan_in_feat(y, x, name)


def _nan_in_feat(y, x, name):
    feat, other, g = _inputs(name)
    clean = _run(feat, other, g, name)
    assert all(np.isfinite(a).all() for a in clean)
    feat[IMG, 1, y, x] = np.nan
    out, prob, df, do = _run(feat, other, g, name)
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


def test_a_nan_in_other_reaches_every_pixel_of_its_image():
    for name in NAMES:
        for y, x in PLACES:
            _nan_in_other(y, x, name)


def _nan_in_other(y, x, name):
    feat, other, g = _inputs(name)
    clean = _run(feat, other, g, name)
    other[IMG, 2, y, x] = np.nan
    res = _run(feat, other, g, name)
    for what, got, ref in zip(("forward", "prob", "d feat", "d other"), res, clean):
        bad = np.zeros(got.shape, bool)
        bad[IMG] = True
        _check(what, got, ref, bad)


def test_an_infinite_feature_gives_nan_at_plus_inf_and_a_weight_of_zero_at_minus_inf():
    for name in NAMES:
        for value in (np.inf, -np.inf):
            for y, x in PLACES:
                _infinite(y, x, value, name)


def _infinite(y, x, value, name):
    """other_0(q) = +-inf: the logit of p at q is +inf where value * feat_0(p) > 0 (inf - inf: NaN), NaN where feat_0(p) = 0 (0 * inf in a
    real channel) and -inf where it is < 0: a weight of exactly 0 -- at q = 0 too, on this route -- so that the pixel stays finite and is
    the float64 evaluation of the frame in which q counts for nothing (other_0(q) = +-60000: logits below -540), within the forward's bar"""
    feat, other, g = _inputs(name)
    clean = _run(feat, other, g, name)
    other[IMG, 0, y, x] = value
    out, prob, df, do = _run(feat, other, g, name)
    for got, ref in zip((out, prob, df, do), clean):
        assert np.array_equal(got[1 - IMG].view(np.uint32), ref[1 - IMG].view(np.uint32))
    zero = feat[IMG, 0] * np.float32(np.sign(value)) < 0                                     # the pixels whose logit at q is -inf
    assert zero.any() and (~zero).any()
    assert np.isnan(out[IMG][:, ~zero]).all() and np.isnan(prob[IMG][~zero]).all()
    assert np.isfinite(out[IMG][:, zero]).all() and np.isfinite(prob[IMG][zero]).all()
    other[IMG, 0, y, x] = np.sign(value) * 60000.0
    want = xo.compute(feat, other, -1.0, ignore=y * W + x)
    assert (want['w'][IMG].reshape(H, W, H * W)[zero][:, y * W + x] < 1e-200).all()
    frac = (np.abs(out[IMG][:, zero] - want['out'][IMG][:, zero]) / want['bar'][IMG][:, zero]).max()
    print("%s %s at (%d, %d): the finite pixels are at %.4f of the bar" % (name, value, y, x, frac))
    assert frac <= 1.0
    # d feat: NaN at the pixels that are, and in channel 0 wherever dss = 0 meets the infinite other_0(q); finite elsewhere
    assert np.isnan(df[IMG][:, ~zero]).all() and np.isnan(df[IMG][0]).all() and np.isfinite(df[IMG][1:][:, zero]).all()
    assert np.isnan(do[IMG]).all()                                                           # every p reaches every q


def test_subnormal_inputs_count_at_their_value():
    for name in NAMES:
        _subnormal(name)


def _subnormal(name):
    n, c, h, w = 1, 1, 5, 7
    tiny, big = (1023 * 2.0 ** -24, 65504.0) if name == 'fp16' else (127 * 2.0 ** -133, 2.0 ** 127)
    feat = np.full((n, c, h, w), tiny, np.float32)
    other = np.zeros((n, c, h, w), np.float32)
    other[0, 0, h - 1, w - 1] = big
    dtype = xo.DTYPES[name]
    (f16, fup), (o16, oup) = xo.to16(feat, dtype), xo.to16(other, dtype)
    assert np.array_equal(fup, feat) and np.array_equal(oup, other)                          # both exact in the dtype
    assert float(f16.flatten()[0]) < torch.finfo(dtype).tiny                                 # ... and subnormal in it
    from oflibpytorch_amd import _matching
    out, prob, _ = _matching.flow_global_match_x16(f16.to(_dev()), o16.to(_dev()), -1.0, True, False)
    out = out.cpu().numpy()
    kept, flushed = xo.compute(fup, oup, -1.0), xo.compute(np.zeros_like(fup), oup, -1.0)
    assert np.abs(kept['out'] - flushed['out']).max() > 1000 * kept['bar'].max()             # the two readings are far apart
    frac = (np.abs(out - kept['out']) / kept['bar']).max()
    print("%s: logit %.4f; against the subnormal at its value %.4f of the bar, against a flushed one %.3g of it"
          % (name, kept['s'].max(), frac, (np.abs(out - flushed['out']) / flushed['bar']).max()))
    assert frac <= 1.0


def test_the_api_raises_the_constructors_error():
    import oflibpytorch_amd as ofl
    feat, other, _ = _inputs('bf16')
    feat[IMG, 1, 2, 3] = np.nan
    ft, ot = (torch.from_numpy(a).bfloat16().to(_dev()) for a in (feat, other))
    with pytest.raises(ValueError, match="Error setting flow vectors"):
        ofl.Flow.from_matching(ft, ot, 's')
