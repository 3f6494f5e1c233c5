"""GPU tier of Flow.from_matching (ofl_matching.hip) against tests/matching_oracle.py.

Frames (matching_oracle.frames()), by Q = H W: 1 (the flow is exactly 0 and prob exactly 1); 1 x 5 and 5 x 1, below a wave; the kernel's
p-tile (64), q-chunk (32) and the four chunks a gradient block walks at a time (128), each minus one, exact and plus one; two of each plus
one; a batch of 3.  Channels (matching_oracle.channels()): 1, the channel chunk minus one, itself, plus one, twice plus three; for the
gradients also C around the 32 channels of a wave and the 128 of a walk, and two walks plus three.  Both refs.

BIT FOR BIT (for any correct exp: exp(0) = 1 and exp(-1024) = +0 exactly): the forward, prob, d feat and d other equal the oracle on
features in {0, +-32} with C = 16 or 4, whose logits are 0 or at most -1024 -- one-hot (each p matches one named q, planted on both sides
of the chunk and tile borders, the first and the last q included), two-hot (weights of exactly 1/2, the two matches in different chunks),
all-equal (every weight 1 / Q) and a maximum that rises twice along the walk by 1024 (the rescale at exactly 0).

GENERAL: features N(0, 1) on a grid of 2^-6.  The kernel and the oracle take the same IEEE steps in the same order and differ in exp
alone, each within 1 ulp64 of the true value.
  forward   held to ulp32(want) + 2^-k A against the definition before its last rounding, A = sum_q w |q - p|.  A term e_q differs by at
            most 2^-51 of itself, and so does every rescale factor it has passed through, at most Q - 1 of them: 2^-51 Q per term.
            d ox = sum_q w_q delta_q (qx - ox) and |qx - ox| <= |qx - x| + A give 2 A 2^-51 Q; the margin is 16 x:
            k = 51 - 1 - ceil(log2 Q) - 4 = 46 - ceil(log2 Q) (39 at Q = 65, 36 at Q = 560); the ulp32 covers the one float32 rounding
            falling on either side.
  gradients held to ulp32(want) + 2^-k A against the float64 sum of the definition's float32 terms dss * other_c (dss * feat_c), A the
            sum of their absolute values.  The ACCUMULATOR IS FLOAT32 (one per element, the order of the definition): the float32
            product costs 2^-24 of a term, the sum of Q terms (Q - 1) 2^-24 A, and the three roundings to float32 a term passes (ds, its
            division by the root, the product) can each be moved to the neighbouring float32 by the difference in exp, 2^-23 of the
            term each: under (Q + 6) 2^-24 A; the margin is 16 x: k = 24 - ceil(log2(Q + 6)) - 4 (13 at Q = 65, 10 at Q = 560).
Every test prints the worst fraction of its bar before it asserts."""
import functools

import numpy as np
import pytest
import torch

import matching_oracle as mo

gpu = pytest.mark.gpu
FRAMES = mo.frames()
CHANNELS = mo.channels()
SIGN = {'s': -1.0, 't': 1.0}


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
    """|got - want| <= ulp32(want) + 2^-shift A, element by element; returns the worst fraction of the bar"""
    got = np.ascontiguousarray(got)
    assert got.dtype == np.float32 and got.shape == want64.shape, (what, got.dtype, got.shape, want64.shape)
    bar = mo.ulp32(want64) + 2.0 ** -shift * mag
    err = np.abs(got.astype(np.float64) - want64)
    frac = float((err / bar).max())
    print("%s: worst error %.3f of the bar ulp32 + 2^-%d A" % (what, frac, shift))
    assert np.isfinite(got).all() and frac <= 1.0, (what, frac)
    return frac


@functools.lru_cache(maxsize=None)
def _want(kind, n, c, h, w, ref):
    """The oracle's results, computed once per case and left unchanged"""
    feat, other = mo.features_general(n, c, h, w) if kind == "general" else mo.features_exact(kind, n, c, h, w)
    g = mo.upstream(n, h, w)
    return feat, other, g, mo.compute(feat, other, SIGN[ref]), mo.grads(feat, other, SIGN[ref], g)


def _run(feat, other, g, ref):
    from oflibpytorch_amd import _matching, _native
    n, c, h, w = feat.shape
    ft, ot = _to(feat), _to(other)
    out, prob, stats = _matching.flow_global_match(ft, ot, SIGN[ref], True, True)
    assert 'flow_global_match_kernel' in _native.last_kernel_name()
    assert out.dtype == torch.float32 and out.shape == (n, 2, h, w) and out.is_contiguous()
    assert prob.dtype == torch.float32 and prob.shape == (n, h, w) and prob.is_contiguous()
    assert stats.dtype == torch.uint8 and stats.numel() == 28 * n * h * w
    df, do = _matching.flow_global_match_grad(ft, ot, SIGN[ref], stats, _to(g))
    assert 'flow_global_match_grad_kernel' in _native.last_kernel_name()
    for d in (df, do):
        assert d.dtype == torch.float32 and d.shape == (n, c, h, w) and d.is_contiguous()
    return out.cpu().numpy(), prob.cpu().numpy(), df.cpu().numpy(), do.cpu().numpy(), stats


def _stats(stats, n, q):
    """(m float32 [n, q]; S, ox, oy float64 [n, q]) out of the workspace"""
    raw = stats.cpu().numpy()
    d = raw[:24 * n * q].view(np.float64).reshape(3, n, q)
    return raw[24 * n * q:].view(np.float32).reshape(n, q), d[0], d[1], d[2]


# ---- bar 1: bit for bit on features whose softmax is exact ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,h,w", FRAMES, ids=_ids(FRAMES))
def test_exact_softmax_bit_for_bit(n, h, w):
    for c, kinds in ((16, ('one-hot', 'two-hot', 'all-equal', 'rising')), (4, ('one-hot', 'all-equal'))):
        for kind in kinds:
            for ref in ('s', 't'):
                feat, other, g, fwd, gr = _want(kind, n, c, h, w, ref)
                what = "%d x %d x %d C %d %s %s" % (n, h, w, c, kind, ref)
                out, prob, df, do, stats = _run(feat, other, g, ref)
                same_bits(out, fwd['out32'], what + ": forward")
                same_bits(prob, fwd['prob'], what + ": prob")
                m, S, ox, oy = _stats(stats, n, h * w)
                assert np.array_equal(m, fwd['m']) and np.array_equal(S, fwd['S']), what + ": the saved maximum and sum"
                assert np.array_equal(ox, fwd['ox']) and np.array_equal(oy, fwd['oy']), what + ": the saved expectation"
                same_bits(df, gr['d_feat'], what + ": d feat")
                same_bits(do, gr['d_other'], what + ": d other")
    if h * w == 1:
        assert not out.any() and np.array_equal(prob, np.ones((n, 1, 1), np.float32))           # 1 x 1: the flow is exactly 0
    else:
        assert np.abs(_want('one-hot', n, 16, h, w, 's')[3]['out']).max() >= 1


# ---- bar 2: general features within the derived bars -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("n,h,w", FRAMES, ids=_ids(FRAMES))
def test_general_features_within_the_bars(n, h, w, c):
    q = h * w
    for ref in ('s', 't'):
        feat, other, g, fwd, gr = _want("general", n, c, h, w, ref)
        what = "%d x %d x %d C %d %s" % (n, h, w, c, ref)
        out, prob, df, do, _ = _run(feat, other, g, ref)
        within(out, fwd['out'], fwd['mag'], mo.forward_shift(q), what + ": forward")
        within(prob, 1.0 / fwd['S'].reshape(n, h, w), 1.0 / fwd['S'].reshape(n, h, w), mo.forward_shift(q), what + ": prob")
        within(df, gr['d_feat64'], gr['mag_feat'], mo.grad_shift(q), what + ": d feat")
        within(do, gr['d_other64'], gr['mag_other'], mo.grad_shift(q), what + ": d other")
    assert q == 1 or (np.abs(gr['d_feat64']).max() > 1e-4 and np.abs(gr['d_other64']).max() > 1e-4)


@gpu
@pytest.mark.parametrize("c", mo.grad_channels())
def test_gradient_channel_groups_within_the_bars(c):
    """A wave of a gradient block sums kGradChan channels, a block kGradWaves of them per walk: C around both, and two walks plus three, on
    a frame of two tiles and four chunks plus one (3 x 43)"""
    n, h, w = 1, 3, 43
    feat, other, g, fwd, gr = _want("general", n, c, h, w, 's')
    what = "%d x %d x %d C %d" % (n, h, w, c)
    out, prob, df, do, _ = _run(feat, other, g, 's')
    within(out, fwd['out'], fwd['mag'], mo.forward_shift(h * w), what + ": forward")
    within(df, gr['d_feat64'], gr['mag_feat'], mo.grad_shift(h * w), what + ": d feat")
    within(do, gr['d_other64'], gr['mag_other'], mo.grad_shift(h * w), what + ": d other")
    # ... and bit for bit: the float32 sums of the definition, whenever no float32 rounding of a term was moved by the device's exp
    moved = int((df.view(np.uint32) != gr['d_feat'].view(np.uint32)).sum() + (do.view(np.uint32) != gr['d_other'].view(np.uint32)).sum())
    print("%s: %d of %d gradient elements differ from the oracle's float32 sums in any bit" % (what, moved, df.size + do.size))


# ---- bar 3: the same bits on any run, in any batch, with one gradient alone -------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", [3, 16])
def test_one_gradient_alone_a_repeat_and_a_batch_give_the_same_bits(c):
    from oflibpytorch_amd import _matching
    n, h, w = 3, 7, 19                                                                       # Q = 133: three tiles, five chunks
    feat, other = mo.features_general(n, c, h, w)
    ft, ot, gt = _to(feat), _to(other), _to(mo.upstream(n, h, w))
    bits = lambda t: t.view(torch.int32)
    out, prob, stats = _matching.flow_global_match(ft, ot, -1.0, True, True)
    df, do = _matching.flow_global_match_grad(ft, ot, -1.0, stats, gt)
    bare, none, nothing = _matching.flow_global_match(ft, ot, -1.0, False, False)
    assert none is None and nothing is None and torch.equal(bits(bare), bits(out))
    only_f, none = _matching.flow_global_match_grad(ft, ot, -1.0, stats, gt, want_other=False)
    assert none is None and torch.equal(bits(only_f), bits(df))
    none, only_o = _matching.flow_global_match_grad(ft, ot, -1.0, stats, gt, want_feat=False)
    assert none is None and torch.equal(bits(only_o), bits(do))
    o2, p2, s2 = _matching.flow_global_match(ft, ot, -1.0, True, True)
    assert torch.equal(bits(o2), bits(out)) and torch.equal(bits(p2), bits(prob)) and torch.equal(s2, stats)
    again = _matching.flow_global_match_grad(ft, ot, -1.0, s2, gt)
    assert torch.equal(bits(again[0]), bits(df)) and torch.equal(bits(again[1]), bits(do))
    for b in range(n):
        o1, p1, s1 = _matching.flow_global_match(ft[b:b + 1], ot[b:b + 1], -1.0, True, True)
        assert torch.equal(bits(o1[0]), bits(out[b])) and torch.equal(bits(p1[0]), bits(prob[b]))
        f1, g1 = _matching.flow_global_match_grad(ft[b:b + 1], ot[b:b + 1], -1.0, s1, gt[b:b + 1].contiguous())
        assert torch.equal(bits(f1[0]), bits(df[b])) and torch.equal(bits(g1[0]), bits(do[b]))
        o3, _, _ = _matching.flow_global_match(ft[b], ot[b], -1.0)                           # C-H-W: a batch of one
        assert torch.equal(bits(o3[0]), bits(out[b]))


# ---- bar 4: the volume is never formed -----------------------------------------------------------------------------------------------------
@gpu
def test_peak_memory_stays_far_below_the_volume():
    """N = 2, C = 16, 40 x 48: the volume is 14.7 MB per image.  Across a forward plus backward through Flow.from_matching the peak
    beyond the inputs stays under 1/16 of ONE image's volume (0.92 MB): outputs, workspace and gradients are about 0.4 MB.  A condition,
    not a measurement."""
    import oflibpytorch_amd as ofl
    n, c, h, w = 2, 16, 40, 48
    rng = np.random.RandomState(3)
    ft = _to(rng.normal(size=(n, c, h, w)).astype(np.float32)).requires_grad_(True)
    ot = _to(rng.normal(size=(n, c, h, w)).astype(np.float32)).requires_grad_(True)
    gt = _to(rng.normal(size=(n, 2, h, w)).astype(np.float32))
    ofl.Flow.from_matching(ft.detach(), ot.detach(), 's')                                   # (the library is loaded, the first launch made)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    flow, prob = ofl.Flow.from_matching(ft, ot, 's', return_prob=True)
    flow.vecs.backward(gt)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    volume = 4 * (h * w) ** 2
    print("peak beyond the inputs: %d bytes = 1 / %.1f of one image's volume of %d bytes" % (peak, volume / max(peak, 1), volume))
    assert ft.grad is not None and ot.grad is not None
    assert peak < volume // 16


# ---- bar 5: the whole API ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ref", ['s', 't'])
def test_the_api_and_its_backward_against_the_bindings(ref):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _matching
    n, c, h, w = 2, 5, 20, 28
    feat, other, g, fwd, gr = _want("general", n, c, h, w, ref)
    ft, ot, gt = _to(feat).requires_grad_(True), _to(other).requires_grad_(True), _to(g)
    mask = torch.rand(n, h, w, device=_dev()) > 0.3
    flow, prob = ofl.Flow.from_matching(ft, ot, ref, mask, return_prob=True)
    assert isinstance(flow, ofl.Flow) and flow.ref == ref and flow.shape == (n, h, w) and flow.device == ft.device
    assert torch.equal(flow.mask, mask)
    assert flow.vecs.requires_grad and type(flow.vecs.grad_fn).__name__ == "GlobalMatchFnBackward"
    assert prob.dtype == torch.float32 and prob.shape == (n, h, w) and not prob.requires_grad
    what = "Flow.from_matching %s" % ref
    within(flow.vecs.detach().cpu().numpy(), fwd['out'], fwd['mag'], mo.forward_shift(h * w), what + ": forward")
    within(prob.cpu().numpy(), 1.0 / fwd['S'].reshape(n, h, w), 1.0 / fwd['S'].reshape(n, h, w), mo.forward_shift(h * w), what + ": prob")
    flow.vecs.backward(gt)
    within(ft.grad.cpu().numpy(), gr['d_feat64'], gr['mag_feat'], mo.grad_shift(h * w), what + ": d feat")
    within(ot.grad.cpu().numpy(), gr['d_other64'], gr['mag_other'], mo.grad_shift(h * w), what + ": d other")
    # .grad is what the binding gives, bit for bit
    out, _, stats = _matching.flow_global_match(ft.detach(), ot.detach(), SIGN[ref], False, True)
    df, do = _matching.flow_global_match_grad(ft.detach(), ot.detach(), SIGN[ref], stats, gt)
    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(out), bits(flow.vecs.detach())) and torch.equal(bits(df), bits(ft.grad)) and torch.equal(bits(do), bits(ot.grad))
    # one operand alone: only the wanted gradient is computed
    calls = []
    real = _matching.flow_global_match_grad

    def spy(*args, **kw):
        calls.append((kw["want_feat"], kw["want_other"]))
        return real(*args, **kw)
    _matching.flow_global_match_grad = spy
    try:
        f2 = ft.detach().clone().requires_grad_(True)
        ofl.Flow.from_matching(f2, ot.detach(), ref).vecs.backward(gt)
        o2 = ot.detach().clone().requires_grad_(True)
        ofl.Flow.from_matching(ft.detach(), o2, ref).vecs.backward(gt)
    finally:
        _matching.flow_global_match_grad = real
    assert calls == [(True, False), (False, True)]
    assert torch.equal(bits(f2.grad), bits(df)) and torch.equal(bits(o2.grad), bits(do))
    # without a gradient: the same bits, no graph; the tensor wrapper likewise
    bare = ofl.Flow.from_matching(ft.detach(), ot.detach(), ref)
    assert not bare.vecs.requires_grad and torch.equal(bits(bare.vecs), bits(out)) and bool(bare.mask.all())
    got = ofl.global_matching_flow(ft.detach(), ot.detach(), ref)
    assert got.shape == (n, 2, h, w) and torch.equal(bits(got), bits(out))
