"""GPU tier of Flow.propagate (ofl_propagate.hip) against tests/propagate_oracle.py.

Global frames (propagate_oracle.global_frames()), by Q = H W: 1; 1 x 5 and 5 x 1; the q-chunk (32), the p-tile (64) and the four chunks a
gradient block walks at a time (128), each minus one, exact, plus one and twice plus one; a batch of 3.  Local frames
(propagate_oracle.local_frames()), every radius 1 .. 4: 1 x 1, 1 x 7, 7 x 1 and 2 x 3, smaller than the window; the tile's width (32) and
height (4), each minus one, exact, plus one and twice plus one; a batch of 3.  Masks (propagate_oracle.masks()): none; single excluded
positions at the first and last q and on either side of every chunk and tile border; a checkerboard; one image fully masked, whose pixels
are empty; for the local form a masked block wider than the window, with empty pixels inside.

BIT FOR BIT (for any correct exp: exp(0) = 1 and exp(-1024) = +0 exactly): the forward, the saved statistics, the result mask and all
three gradients equal the oracle on features in {0, +-32} with C = 16 or 4, whose logits -- and whose differences, the padded logit +0
included, which ties with the maximum -- are 0 or at most -1024, and vectors on a grid of 2^-6.

GENERAL: features N(0, 1) on a grid of 2^-6.  The kernel and the oracle take the same IEEE steps in the same order and differ in exp
alone, each within 1 ulp64 of the true value.
  forward   held to ulp32(want) + 2^-k A against the definition before its last rounding, A = sum_q w |value(q) - out(p)|,
            k = 46 - ceil(log2 T), T the participating positions of the pixel: the derivation of test_gpu_matching.py with values in
            place of coordinates (|value - out| enters A directly); the local form has no rescale and stays inside it.
  gradients held to ulp32(want) + 2^-k A against the float64 sum of the definition's float32 terms, A the sum of their absolute values,
            k = 20 - ceil(log2(T + 6)), T the number of terms of the element: the float32 product, the float32 sum of T terms and three
            float32 roundings per term that the difference in exp may move, with a margin of 16 (test_gpu_matching.py).
Every test prints the worst fraction of its bar before it asserts."""
import functools

import numpy as np
import pytest
import torch

import propagate_oracle as po

gpu = pytest.mark.gpu
GLOBAL_FRAMES = po.global_frames()
LOCAL_FRAMES = po.local_frames()
LOCAL_GENERAL = [(1, 2, 3), (1, 3, po.geometry()["kLTileW"] + 1), (1, 2 * po.geometry()["kLTileH"] + 1, 5), (3, 5, 7)]
RADII = (1, 2, 3, 4)


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _ids(frames):
    return ["%dx%dx%d" % f for f in frames]


def _to(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x).copy()).to(_dev())


def same_bits(got, want, what):
    """Equal bit for bit; where both are NaN the payload is exempt"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        at = tuple(int(i[0]) for i in np.nonzero(bad))
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, expected %r" % (what, int(bad.sum()), bad.size, at,
                                                                                                 got[at], want[at]))


def within(got, want64, mag, shift, what):
    """|got - want| <= ulp32(want) + 2^-shift A, element by element (`shift` an array that broadcasts); returns the worst fraction"""
    got = np.ascontiguousarray(got)
    assert got.dtype == np.float32 and got.shape == want64.shape, (what, got.dtype, got.shape, want64.shape)
    bar = po.ulp32(want64) + 2.0 ** -np.asarray(shift, np.float64) * mag
    err = np.abs(got.astype(np.float64) - want64)
    frac = float((err / bar).max())
    print("%s: worst error %.3f of the bar ulp32 + 2^-k A, smallest k %d" % (what, frac, int(np.min(shift))))
    assert np.isfinite(got).all() and frac <= 1.0, (what, frac)
    return frac


def stats_of(stats, n, q):
    """(m float32 [n, q]; S, ox, oy float64 [n, q]) out of the workspace"""
    raw = stats.cpu().numpy()
    d = raw[:24 * n * q].view(np.float64).reshape(3, n, q)
    return raw[24 * n * q:].view(np.float32).reshape(n, q), d[0], d[1], d[2]


@functools.lru_cache(maxsize=None)
def _want(kind, mask_name, n, c, h, w, radius):
    """The oracle's results, computed once per case and left unchanged"""
    query, key = po.features_general(n, c, h, w) if kind == "general" else po.features_exact(kind, n, c, h, w)
    flow, g, mask = po.vectors(n, h, w), po.upstream(n, h, w), po.masks(n, h, w, radius)[mask_name]
    return flow, mask, query, key, g, po.compute(flow, mask, query, key, radius), po.grads(flow, mask, query, key, radius, g)


def run(flow, mask, query, key, radius, g):
    from oflibpytorch_amd import _native, _propagate
    n, c, h, w = query.shape
    ft, mt, qt, kt = _to(flow), _to(mask), _to(query), _to(key)
    out, valid, stats = _propagate.flow_propagate(ft, mt, qt, kt, radius, True)
    assert ('flow_propagate_global_kernel' if radius is None else 'flow_propagate_local_kernel') in _native.last_kernel_name()
    assert out.dtype == torch.float32 and out.shape == (n, 2, h, w) and out.is_contiguous()
    assert (valid is None) == (mask is None) and (valid is None or (valid.dtype == torch.bool and valid.shape == (n, h, w)))
    assert stats.dtype == torch.uint8 and stats.numel() == 28 * n * h * w
    dq, dk, df = _propagate.flow_propagate_grad(ft, mt, qt, kt, radius, stats, _to(g))
    assert ('flow_propagate_global_grad_kernel' if radius is None else 'flow_propagate_local_gather_kernel') in _native.last_kernel_name()
    for d, ch in ((dq, c), (dk, c), (df, 2)):
        assert d.dtype == torch.float32 and d.shape == (n, ch, h, w) and d.is_contiguous()
    return (out.cpu().numpy(), None if valid is None else valid.cpu().numpy(), stats, dq.cpu().numpy(), dk.cpu().numpy(), df.cpu().numpy())


def _bit_for_bit(n, h, w, radius):
    empties = 0
    for c in (16, 4):
        for kind in po.exact_kinds(c):
            for mask_name in po.masks(n, h, w, radius):
                flow, mask, query, key, g, fwd, gr = _want(kind, mask_name, n, c, h, w, radius)
                what = "%d x %d x %d r %s C %d %s mask %s" % (n, h, w, radius, c, kind, mask_name)
                out, valid, stats, dq, dk, df = run(flow, mask, query, key, radius, g)
                same_bits(out, fwd['out32'], what + ": forward")
                assert mask is None or np.array_equal(valid, fwd['valid']), what + ": the result mask"
                m, S, ox, oy = stats_of(stats, n, h * w)
                assert np.array_equal(m, fwd['m']) and np.array_equal(S, fwd['S']), what + ": the saved maximum and sum"
                assert np.array_equal(ox, fwd['ox']) and np.array_equal(oy, fwd['oy']), what + ": the saved expectation"
                same_bits(dq, gr['d_query'], what + ": d query")
                same_bits(dk, gr['d_key'], what + ": d key")
                same_bits(df, gr['d_flow'], what + ": d flow")
                empties += int((~fwd['valid']).sum())
    return empties


# ---- bar 1: bit for bit on features whose softmax is exact ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,h,w", GLOBAL_FRAMES, ids=_ids(GLOBAL_FRAMES))
def test_global_exact_softmax_bit_for_bit(n, h, w):
    assert _bit_for_bit(n, h, w, None) > 0                                                  # (the fully masked image: empty pixels)
    if h * w > 1:
        assert np.abs(_want('one-hot', 'none', n, 16, h, w, None)[5]['out']).max() >= 0.5


@gpu
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("n,h,w", LOCAL_FRAMES, ids=_ids(LOCAL_FRAMES))
def test_local_exact_softmax_bit_for_bit(n, h, w, radius):
    assert _bit_for_bit(n, h, w, radius) > 0
    if h >= 2 * radius + 3 and w >= 2 * radius + 3:                                         # the masked block holds a pixel whose whole window it covers
        assert not _want('all-equal', 'block', n, 16, h, w, radius)[5]['valid'][:, radius + 1, radius + 1].any()


# ---- bar 2: general features within the derived bars -----------------------------------------------------------------------------------
def _general(n, h, w, c, radius, mask_names):
    worst = {}
    for mask_name in mask_names:
        flow, mask, query, key, g, fwd, gr = _want("general", mask_name, n, c, h, w, radius)
        what = "%d x %d x %d r %s C %d mask %s" % (n, h, w, radius, c, mask_name)
        out, valid, _, dq, dk, df = run(flow, mask, query, key, radius, g)
        assert mask is None or np.array_equal(valid, fwd['valid'])
        fr = {'forward': within(out, fwd['out'], fwd['mag'], po.forward_shift(fwd['terms'])[:, None], what + ": forward")}
        for name, got in (('d_query', dq), ('d_key', dk), ('d_flow', df)):
            fr[name] = within(got, gr[name + '64'], gr['mag_' + name], po.grad_shift(gr['terms_' + name]), what + ": " + name)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in fr.items()}
    return worst


@gpu
@pytest.mark.parametrize("c", po.channels(None))
@pytest.mark.parametrize("n,h,w", GLOBAL_FRAMES, ids=_ids(GLOBAL_FRAMES))
def test_global_general_features_within_the_bars(n, h, w, c):
    _general(n, h, w, c, None, ('none', 'checker', 'single'))


@gpu
@pytest.mark.parametrize("c", po.channels(1))
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("n,h,w", LOCAL_GENERAL, ids=_ids(LOCAL_GENERAL))
def test_local_general_features_within_the_bars(n, h, w, radius, c):
    _general(n, h, w, c, radius, ('none', 'checker', 'block'))


@gpu
@pytest.mark.parametrize("c", po.grad_channels())
def test_gradient_channel_groups_within_the_bars(c):
    """A wave of a global gradient block sums kGradChan channels, a block kGradWaves of them per walk: C around both, and two walks plus
    three, on a frame of two tiles and four chunks plus one (3 x 43); the local form walks any C in chunks of kLChan (r = 2)"""
    _general(1, 3, 43, c, None, ('checker',))
    _general(1, 3, 43, c, 2, ('checker',))


# ---- bar 3: the same bits on any run, in any batch, with one gradient alone -------------------------------------------------------------
@gpu
@pytest.mark.parametrize("radius", [None, 2])
@pytest.mark.parametrize("c", [3, 16])
def test_one_gradient_alone_a_repeat_and_a_batch_give_the_same_bits(c, radius):
    from oflibpytorch_amd import _propagate
    n, h, w = 3, 7, 19                                                                       # Q = 133: three tiles, five chunks
    query, key = po.features_general(n, c, h, w)
    ft, qt, kt, gt = _to(po.vectors(n, h, w)), _to(query), _to(key), _to(po.upstream(n, h, w))
    mt = _to(po.masks(n, h, w, radius)['checker'])
    bits = lambda t: t.view(torch.int32)
    fwd, bwd = _propagate.flow_propagate, _propagate.flow_propagate_grad
    out, valid, stats = fwd(ft, mt, qt, kt, radius, True)
    grads = bwd(ft, mt, qt, kt, radius, stats, gt)
    bare, v2, nothing = fwd(ft, mt, qt, kt, radius, False)
    assert nothing is None and torch.equal(bits(bare), bits(out)) and torch.equal(v2, valid)
    for i in range(3):                                                                       # one gradient alone
        wants = [j == i for j in range(3)]
        only = bwd(ft, mt, qt, kt, radius, stats, gt, *wants)
        assert [o is not None for o in only] == wants and torch.equal(bits(only[i]), bits(grads[i]))
    o2, _, s2 = fwd(ft, mt, qt, kt, radius, True)                                            # a repeat
    assert torch.equal(bits(o2), bits(out)) and torch.equal(s2, stats)
    again = bwd(ft, mt, qt, kt, radius, s2, gt)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(again, grads))
    for b in range(n):                                                                       # the image alone
        one = lambda t: t[b:b + 1].contiguous()
        o1, v1, s1 = fwd(one(ft), one(mt), one(qt), one(kt), radius, True)
        assert torch.equal(bits(o1[0]), bits(out[b])) and torch.equal(v1[0], valid[b])
        g1 = bwd(one(ft), one(mt), one(qt), one(kt), radius, s1, one(gt))
        assert all(torch.equal(bits(a[0]), bits(x[b])) for a, x in zip(g1, grads))
        o3, _, s3 = fwd(one(ft), one(mt), qt[b], kt[b], radius, True)                        # C-H-W operands: one image for the batch
        assert torch.equal(bits(o3[0]), bits(out[b]))
        g3 = bwd(one(ft), one(mt), qt[b], kt[b], radius, s3, one(gt))
        assert all(torch.equal(bits(a[0]), bits(x[b])) for a, x in zip(g3, grads))


# ---- bar 4: the volume is never formed -----------------------------------------------------------------------------------------------------
@gpu
def test_peak_memory_stays_far_below_the_volume():
    """N = 2, C = 16, 40 x 48: the volume is 14.7 MB per image.  Across a global forward plus backward through Flow.propagate the peak
    beyond the inputs stays under 1/8 of ONE image's volume (1.84 MB): result, statistics and gradients are about 0.7 MB.  A condition,
    not a measurement."""
    import oflibpytorch_amd as ofl
    n, c, h, w = 2, 16, 40, 48
    rng = np.random.RandomState(3)
    qt = _to(rng.normal(size=(n, c, h, w)).astype(np.float32)).requires_grad_(True)
    kt = _to(rng.normal(size=(n, c, h, w)).astype(np.float32)).requires_grad_(True)
    vt = _to(rng.normal(size=(n, 2, h, w)).astype(np.float32)).requires_grad_(True)
    gt = _to(rng.normal(size=(n, 2, h, w)).astype(np.float32))
    mt = _to(rng.uniform(size=(n, h, w)) > 0.3)
    flow = ofl.Flow(vt, 't', mt)
    flow.propagate(qt.detach(), kt.detach())                                                 # (the library is loaded, the first launch made)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = flow.propagate(qt, kt)
    res.vecs.backward(gt)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    volume = 4 * (h * w) ** 2
    print("peak beyond the inputs: %d bytes = 1 / %.1f of one image's volume of %d bytes" % (peak, volume / max(peak, 1), volume))
    assert qt.grad is not None and kt.grad is not None and vt.grad is not None
    assert peak < volume // 8


# ---- bar 5: the whole API ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("radius", [None, 3])
def test_the_api_and_its_backward_against_the_bindings(radius):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _propagate
    n, c, h, w = 2, 5, 20, 28
    flow, mask, query, key, g, fwd, gr = _want("general", "checker", n, c, h, w, radius)
    vt, qt, kt, gt, mt = _to(flow).requires_grad_(True), _to(query).requires_grad_(True), _to(key).requires_grad_(True), _to(g), _to(mask)
    res = ofl.Flow(vt, 's', mt).propagate(qt, kt, radius)
    assert isinstance(res, ofl.Flow) and res.ref == 's' and res.shape == (n, h, w) and res.device == qt.device
    assert bool(res.mask.all())
    assert res.vecs.requires_grad and type(res.vecs.grad_fn).__name__ == "PropagateFnBackward"
    what = "Flow.propagate r %s" % radius
    within(res.vecs.detach().cpu().numpy(), fwd['out'], fwd['mag'], po.forward_shift(fwd['terms'])[:, None], what + ": forward")
    res.vecs.backward(gt)
    for name, t in (('d_query', qt), ('d_key', kt), ('d_flow', vt)):
        within(t.grad.cpu().numpy(), gr[name + '64'], gr['mag_' + name], po.grad_shift(gr['terms_' + name]), what + ": " + name)
    # .grad is what the binding gives, bit for bit
    det = (vt.detach(), mt, qt.detach(), kt.detach())
    out, valid, stats = _propagate.flow_propagate(*det, radius, True)
    dq, dk, df = _propagate.flow_propagate_grad(*det, radius, stats, gt)
    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(out), bits(res.vecs.detach())) and torch.equal(valid, res.mask)
    assert torch.equal(bits(dq), bits(qt.grad)) and torch.equal(bits(dk), bits(kt.grad)) and torch.equal(bits(df), bits(vt.grad))
    # one operand alone: only the wanted gradient is computed
    calls = []
    real = _propagate.flow_propagate_grad

    def spy(*args, **kw):
        calls.append((kw["want_query"], kw["want_key"], kw["want_flow"]))
        return real(*args, **kw)
    _propagate.flow_propagate_grad = spy
    try:
        q2 = qt.detach().clone().requires_grad_(True)
        ofl.Flow(vt.detach(), 's', mt).propagate(q2, kt.detach(), radius).vecs.backward(gt)
        k2 = kt.detach().clone().requires_grad_(True)
        ofl.Flow(vt.detach(), 's', mt).propagate(qt.detach(), k2, radius).vecs.backward(gt)
        v2 = vt.detach().clone().requires_grad_(True)
        ofl.Flow(v2, 's', mt).propagate(qt.detach(), kt.detach(), radius).vecs.backward(gt)
    finally:
        _propagate.flow_propagate_grad = real
    assert calls == [(True, False, False), (False, True, False), (False, False, True)]
    assert torch.equal(bits(q2.grad), bits(dq)) and torch.equal(bits(k2.grad), bits(dk)) and torch.equal(bits(v2.grad), bits(df))
    # key=None equals passing the tensor twice: the same forward bits, and autograd adds the two gradients
    q3, q4 = qt.detach().clone().requires_grad_(True), qt.detach().clone().requires_grad_(True)
    a = ofl.Flow(vt.detach(), 's', mt).propagate(q3, None, radius)
    b = ofl.Flow(vt.detach(), 's', mt).propagate(q4, q4, radius)
    assert torch.equal(bits(a.vecs.detach()), bits(b.vecs.detach()))
    a.vecs.backward(gt)
    b.vecs.backward(gt)
    assert torch.equal(bits(q3.grad), bits(q4.grad))
    d3 = _propagate.flow_propagate_grad(vt.detach(), mt, q3.detach(), q3.detach(), radius,
                                        _propagate.flow_propagate(vt.detach(), mt, q3.detach(), q3.detach(), radius, True)[2], gt)
    assert torch.equal(bits(q3.grad), bits(d3[0] + d3[1]))
    # without a gradient: the same bits, no graph; consider_mask False; the tensor wrapper likewise
    bare = ofl.Flow(vt.detach(), 's', mt).propagate(qt.detach(), kt.detach(), radius)
    assert not bare.vecs.requires_grad and torch.equal(bits(bare.vecs), bits(out))
    free, none, _ = _propagate.flow_propagate(vt.detach(), None, qt.detach(), kt.detach(), radius, False)
    assert none is None
    unmasked = ofl.Flow(vt.detach(), 's', mt).propagate(qt.detach(), kt.detach(), radius, consider_mask=False)
    assert torch.equal(bits(unmasked.vecs), bits(free)) and bool(unmasked.mask.all()) and not torch.equal(bits(free), bits(out))
    got = ofl.propagate_flow(vt.detach(), qt.detach(), kt.detach(), radius)
    assert got.shape == (n, 2, h, w) and torch.equal(bits(got), bits(free))
    got, gv = ofl.propagate_flow(vt.detach(), qt.detach(), kt.detach(), radius, mask=mt)
    assert torch.equal(bits(got), bits(out)) and torch.equal(gv, valid)
