"""Non-finite values through Flow.upsample_convex on the device (ofl_upsample.hip): everything is IEEE as the steps give
it.  A NaN logit, a +inf logit and nine -inf logits make their fine pixel NaN in both channels; a -inf among finite logits is a weight
of exactly 0; a non-finite vector reaches every fine pixel of the up to nine coarse pixels around it, at weight 0 too.  In every case
EXACTLY the stated elements of the forward and of both gradients are non-finite, and every other element carries the bits of the run
without the special (device against device: no bar is involved)."""
import numpy as np
import pytest
import torch

import upsample_convex_oracle as uo

pytestmark = pytest.mark.gpu

N, H, W = 2, 5, 7
IMG = 1                                              # the image that gets the special; the other stays clean


def _to(x):
    return torch.from_numpy(np.ascontiguousarray(x).copy()).to(torch.device('cuda', 0))


def _run(f, lg, g, k, half):
    from oflibpytorch_amd import _upsample
    v = _to(f).half() if half else _to(f)
    out, _ = _upsample.flow_upsample_convex(v, None, _to(lg), k)
    dl, df = _upsample.flow_upsample_convex_grad(v, _to(lg), k, _to(g))
    return out.cpu().numpy(), dl.cpu().numpy(), df.cpu().numpy()


def _check(name, got, clean, bad):
    """Exactly `bad` is non-finite; everything else has the clean run's bits"""
    assert bad.shape == got.shape and bad.any()
    assert np.array_equal(~np.isfinite(got), bad), "%s: %d non-finite elements, %d expected" % (name, (~np.isfinite(got)).sum(), bad.sum())
    assert np.array_equal(got.view(np.uint32)[~bad], clean.view(np.uint32)[~bad]), name + ": an element outside the special's reach changed"


def _around(y, x):
    """The coarse pixels whose 3 x 3 neighbourhood holds (y, x)"""
    return [(yy, xx) for yy in range(max(0, y - 1), min(H, y + 2)) for xx in range(max(0, x - 1), min(W, x + 2))]


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("k", uo.FACTORS)
def test_special_logits(k, half):
    f, _ = uo.case(N, H, W)
    base, g = uo.logits_general(N, k, H, W), uo.upstream(N, k, H, W)
    clean = _run(f, base, g, k, half)
    assert all(np.isfinite(x).all() for x in clean)
    i, j = 1, k - 1
    chan = lambda t: t * k * k + i * k + j
    for (y, x) in ((2, 3), (0, 0), (H - 1, W - 1)):
        for name in ("nan", "+inf", "all -inf"):
            lg = base.copy()
            if name == "nan":
                lg[IMG, chan(5), y, x] = np.nan
            elif name == "+inf":
                lg[IMG, chan(0), y, x] = np.inf
            else:
                lg[IMG, [chan(t) for t in range(9)], y, x] = -np.inf
            out, dl, df = _run(f, lg, g, k, half)
            what = "k %d %s at (%d, %d)" % (k, name, y, x)
            bad = np.zeros(out.shape, bool)
            bad[IMG, :, k * y + i, k * x + j] = True                                          # the fine pixel, both channels
            _check(what + ": forward", out, clean[0], bad)
            assert np.isnan(out[bad]).all()
            bad = np.zeros(dl.shape, bool)
            bad[IMG, [chan(t) for t in range(9)], y, x] = True                                # its nine logits
            _check(what + ": d logits", dl, clean[1], bad)
            bad = np.zeros(df.shape, bool)
            for yy, xx in _around(y, x):                                                      # the vectors it mixes
                bad[IMG, :, yy, xx] = True
            _check(what + ": d flow", df, clean[2], bad)
        # a -inf among finite logits: a weight of exactly 0, everything finite; only what the fine pixel reaches changes
        lg = base.copy()
        lg[IMG, chan(4), y, x] = -np.inf
        out, dl, df = _run(f, lg, g, k, half)
        assert all(np.isfinite(a).all() for a in (out, dl, df))
        assert dl[IMG, chan(4), y, x] == 0.0
        reach = np.zeros(out.shape, bool)
        reach[IMG, :, k * y + i, k * x + j] = True
        assert np.array_equal(out.view(np.uint32)[~reach], clean[0].view(np.uint32)[~reach])
        assert not np.array_equal(out[reach], clean[0][reach])
        reach = np.zeros(dl.shape, bool)
        reach[IMG, [chan(t) for t in range(9)], y, x] = True
        assert np.array_equal(dl.view(np.uint32)[~reach], clean[1].view(np.uint32)[~reach])
        reach = np.zeros(df.shape, bool)
        for yy, xx in _around(y, x):
            reach[IMG, :, yy, xx] = True
        assert np.array_equal(df.view(np.uint32)[~reach], clean[2].view(np.uint32)[~reach])
        want = uo.compute(f, lg, k, float64=True)
        assert np.all(np.abs(out - want['out']) <= uo.ulp32(want['out']) + 2.0 ** -44 * want['mag'])


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("k", uo.FACTORS)
def test_special_vectors(k, half):
    f, _ = uo.case(N, H, W)
    lg, g = uo.logits_general(N, k, H, W), uo.upstream(N, k, H, W)
    clean = _run(f, lg, g, k, half)
    for (y, x) in ((2, 3), (0, 0), (H - 1, 0)):
        for c, value in ((0, np.nan), (1, np.inf), (0, -np.inf)):
            fs = f.copy()
            fs[IMG, c, y, x] = value
            out, dl, df = _run(fs, lg, g, k, half)
            what = "k %d vector %r in channel %d at (%d, %d)" % (k, value, c, y, x)
            bad = np.zeros(out.shape, bool)
            for yy, xx in _around(y, x):                                                      # every fine pixel of the coarse pixels around it,
                bad[IMG, c, k * yy:k * yy + k, k * xx:k * xx + k] = True                      # in the vector's channel
            _check(what + ": forward", out, clean[0], bad)
            bad = np.zeros(dl.shape, bool)
            for yy, xx in _around(y, x):                                                      # all 9 k^2 logits of those coarse pixels
                bad[IMG, :, yy, xx] = True
            _check(what + ": d logits", dl, clean[1], bad)
            # d flow does not depend on the vectors: the clean run's bits everywhere
            assert np.array_equal(df.view(np.uint32), clean[2].view(np.uint32)), what + ": d flow"
