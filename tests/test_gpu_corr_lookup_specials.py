"""Flow.corr_lookup (ofl_corr_lookup.hip) on NaN, +-inf and +-FLT_MAX and on the flow that sends every pixel into one
cell.  The rule of the definition is SELECTION: a node outside the level, and every entry of a pixel that is not usable, is +0 whatever
the features hold; a node inside is read and multiplied whatever its weight.  Everything is also the oracle's bit for bit."""
import numpy as np
import pytest
import torch

import corr_lookup_oracle as cl
from test_gpu_corr_lookup import _grads, _lookup, same_bits

pytestmark = pytest.mark.gpu
N, C, H, W, RADIUS = 2, 3, 20, 28, 2
FLT_MAX = np.finfo(np.float32).max


def _entries_using(a, mask, ref, radius, hl, wl, q):
    """bool [N, D, H, W]: the entries one of whose four nodes is element q of the level, and bool [N, D, H, W]: those with any node inside"""
    win = cl.window(a, mask, ref, 0)
    inside, idx = cl.nodes(win, radius, hl, wl)
    hit = inside & (idx == q) if q is not None else None
    use, some = [], []
    for dx, dy in cl.offsets(radius):
        j, i = dy + radius, dx + radius
        four = [(j, i), (j, i + 1), (j + 1, i), (j + 1, i + 1)]
        some.append(np.any([inside[x] for x in four], 0))
        if hit is not None:
            use.append(np.any([hit[x] for x in four], 0))
    return (np.stack(use, 1) if use else None), np.stack(some, 1)


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("ref", cl.REFS)
def test_a_special_of_other_reaches_the_entries_that_use_its_node_and_no_others(ref, value):
    a, m = cl.case(N, H, W, ref)
    feat, other = cl.features(N, C, H, W, ref), cl.features(N, C, H, W, ref, salt=1).copy()
    q = 2 * W + 2                                                                             # (2, 2): a node of weight 0 of pixel (1, 1), whose position is an integer
    other[:, 1, 2, 2] = value
    use, _ = _entries_using(a, m, ref, RADIUS, H, W, q)
    win = cl.window(a, m, ref, 0)
    assert win['usable'][:, 1, 1].all() and (win['ne'][:, 1, 1] == 0).all() and use[:, :, 1, 1].any() and 0 < use.mean() < 0.5
    out = _lookup((a, m, feat, [other]), ref, RADIUS).cpu().numpy()
    assert np.array_equal(~np.isfinite(out), use)
    same_bits(out, cl.compute(a, m, feat, [other], ref, RADIUS)['lookup'], "a special in `other`")
    # with every pixel whose window covers the node masked, it stays out: forward and both gradients
    covers = use.any(1)
    m2 = m & ~covers
    assert (m & covers).any()
    out = _lookup((a, m2, feat, [other]), ref, RADIUS).cpu().numpy()
    assert np.isfinite(out).all()
    same_bits(out, cl.compute(a, m2, feat, [other], ref, RADIUS)['lookup'], "a special under masked pixels only")
    g = cl.upstream(N, 25, H, W)
    d_feat, (d_other,) = _grads((a, m2, feat, [other]), ref, RADIUS, g)
    want_f, (want_o,) = cl.grads(a, m2, feat, [other], ref, RADIUS, g)
    assert np.isfinite(d_feat.cpu().numpy()).all() and np.isfinite(d_other.cpu().numpy()).all()
    same_bits(d_feat.cpu().numpy(), want_f, "d feat")
    same_bits(d_other.cpu().numpy(), want_o, "d other")


@pytest.mark.parametrize("ref", cl.REFS)
def test_a_nan_in_feat_shows_in_the_entries_of_its_pixel_that_have_a_node_inside(ref):
    a, m = cl.case(N, H, W, ref)
    m = m.copy()
    feat, other = cl.features(N, C, H, W, ref).copy(), cl.features(N, C, H, W, ref, salt=1)
    _, some = _entries_using(a, None, ref, RADIUS, H, W, None)
    # a pixel whose window crosses an edge: some entries have a node inside, some have none
    mixed = some.any(1) & ~some.all(1)
    b, y, x = (int(v[0]) for v in np.nonzero(mixed))
    m[b, y, x] = True
    feat[b, 2, y, x] = np.nan
    expect = np.zeros((N, 25, H, W), bool)
    expect[b, :, y, x] = some[b, :, y, x]
    assert 0 < expect.sum() < 25
    out = _lookup((a, m, feat, [other]), ref, RADIUS).cpu().numpy()
    assert np.array_equal(np.isnan(out), expect)
    assert not out[b, :, y, x][~expect[b, :, y, x]].view(np.uint32).any()                     # the others: +0, selected
    same_bits(out, cl.compute(a, m, feat, [other], ref, RADIUS)['lookup'], "a NaN in feat")


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf, FLT_MAX, -FLT_MAX], ids=["nan", "inf", "-inf", "max", "-max"])
@pytest.mark.parametrize("ref", cl.REFS)
def test_special_vectors_give_zero_everywhere(ref, value):
    feat, lv = cl.explicit_levels(N, C, H, W, ref)
    feat = feat.copy()
    feat[0, 0, 3, 3] = np.nan                                                                 # selected out with the rest
    g = cl.upstream(N, 4 * 25, H, W)
    for comp in (0, 1):
        a = np.array(cl.case(N, H, W, ref)[0])
        a[:, comp] = value
        out = _lookup((a, None, feat, lv), ref, RADIUS).cpu().numpy()
        assert out.shape == (N, 100, H, W) and not out.view(np.uint32).any()
        d_feat, none = _grads((a, None, feat, lv), ref, RADIUS, g, want_levels=[False] * 4)
        assert not d_feat.cpu().numpy().view(np.uint32).any()
        _, d_levels = _grads((a, None, feat, lv), ref, RADIUS, g, want_feat=False)
        for x in d_levels:
            assert not x.cpu().numpy().view(np.uint32).any()


@pytest.mark.parametrize("ref", cl.REFS)
def test_every_pixel_in_one_cell(ref):
    """16 x 32: all 512 windows start in one cell, so each of the (2 r + 2)^2 elements of `other` they cover sums 512 terms in raster
    order and every other element is +0."""
    n, c, h, w, radius = 1, 9, 16, 32, 4
    a, m = cl.one_cell_case(n, h, w, ref)
    feat, other = cl.features(n, c, h, w, ref), cl.features(n, c, h, w, ref, salt=1)
    g = cl.upstream(n, 81, h, w)
    same_bits(_lookup((a, m, feat, [other]), ref, radius).cpu().numpy(), cl.compute(a, m, feat, [other], ref, radius)['lookup'], "the lookup")
    d_feat, (d_other,) = _grads((a, m, feat, [other]), ref, radius, g)
    want_f, (want_o,) = cl.grads(a, m, feat, [other], ref, radius, g)
    same_bits(d_feat.cpu().numpy(), want_f, "d feat")
    same_bits(d_other.cpu().numpy(), want_o, "d other")
    assert (want_o[0, 0] != 0).sum() == 100 and np.abs(want_o).max() > 0.1
    again = _grads((a, m, feat, [other]), ref, radius, g, want_feat=False)[1][0]
    assert torch.equal(again.view(torch.int32), d_other.view(torch.int32))
