"""GPU tier of Flow.upsample_convex (ofl_upsample.hip) against tests/upsample_convex_oracle.py.

Frames (upsample_convex_oracle.frames(), coarse): the kernel's tile -- 64 coarse pixels by 4 fine rows -- minus one, itself, plus one and
two tiles plus one in both axes; 1 x 1, 1 x 5 and 5 x 1, where every or most taps are outside; a batch of 3.  Each at k = 2, 4, 8, with
fp32 and fp16-stored vectors, with and without a mask.

BIT FOR BIT (for any correct exp: exp(0) = 1 and exp(-1000) = +0 exactly): the forward, d logits and d flow equal the oracle on logits that
are constant per fine pixel (0, 3.5, -87), one-hot (0 and -1000: k times one named neighbour, which pins the channel order, the sub-pixel
layout and the border zeros) and two-hot (two weights of exactly 1/2).

GENERAL: logits N(0, 4) on a grid of 2^-6, vectors on a grid of 2^-6 below 32.  The forward is held to ulp32(want) + 2^-44 A with
A = sum_t w_t |F_{c,t}| from the oracle: two exp of <= 1 ulp64, eight adds, a division, nine products and eight adds come to under
2^-48 A, the margin is 16 x, and the ulp32 covers the single float32 rounding falling on either side.  Both gradients are held to
ulp32(want) + 2^-40 A with their own A, the sum of the absolute terms: up to 576 + 30 roundings come to under 2^-43 A, the margin is 16 x.
Every test prints the worst fraction of its bar before it asserts."""
import functools

import numpy as np
import pytest
import torch

import upsample_convex_oracle as uo

gpu = pytest.mark.gpu
FRAMES = uo.frames()
KINDS = ("constant", "one-hot", "two-hot")


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
    bar = uo.ulp32(want64) + 2.0 ** -shift * mag
    err = np.abs(got.astype(np.float64) - want64)
    frac = float((err / bar).max())
    print("%s: worst error %.3f of the bar ulp32 + 2^-%d A" % (what, frac, shift))
    assert np.isfinite(got).all() and frac <= 1.0, (what, frac)
    return frac


@functools.lru_cache(maxsize=None)
def _want(kind, n, k, h, w):
    """The oracle's results, computed once per case and left unchanged"""
    f, _ = uo.case(n, h, w)
    lg = uo.logits_general(n, k, h, w) if kind == "general" else uo.logits_exact(kind, n, k, h, w)
    g = uo.upstream(n, k, h, w)
    fwd = uo.compute(f, lg, k, float64=True)
    gr = uo.grads(f, lg, k, g, float64=True)
    return lg, g, fwd, gr


def _run(n, k, h, w, lg, g, half, masked):
    from oflibpytorch_amd import _native, _upsample
    f, m = uo.case(n, h, w)
    v = _to(f).half() if half else _to(f)
    out, om = _upsample.flow_upsample_convex(v, _to(m) if masked else None, _to(lg), k)
    assert 'flow_upsample_convex_kernel' in _native.last_kernel_name()
    assert out.dtype == torch.float32 and out.shape == (n, 2, k * h, k * w) and out.is_contiguous()
    if masked:
        assert om.dtype == torch.bool and om.shape == (n, k * h, k * w) and om.is_contiguous()
        assert np.array_equal(om.cpu().numpy().view(np.uint8), uo.mask_of(m, k).view(np.uint8))
    else:
        assert om is None
    dl, df = _upsample.flow_upsample_convex_grad(v, _to(lg), k, _to(g))
    assert 'flow_upsample_convex_grad_flow_kernel' in _native.last_kernel_name()
    assert dl.dtype == torch.float32 and dl.shape == (n, 9 * k * k, h, w) and dl.is_contiguous()
    assert df.dtype == torch.float32 and df.shape == (n, 2, h, w) and df.is_contiguous()
    return out.cpu().numpy(), dl.cpu().numpy(), df.cpu().numpy()


# ---- bar 1: bit for bit on logits whose softmax is exact -------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", uo.FACTORS)
@pytest.mark.parametrize("n,h,w", FRAMES, ids=_ids(FRAMES))
def test_exact_logits_bit_for_bit(n, h, w, k):
    for kind in KINDS:
        lg, g, fwd, gr = _want(kind, n, k, h, w)
        for half, masked in ((False, True), (True, False), (False, False), (True, True)):
            what = "%d x %d x %d k %d %s half %s masked %s" % (n, h, w, k, kind, half, masked)
            out, dl, df = _run(n, k, h, w, lg, g, half, masked)
            same_bits(out, fwd['out'].astype(np.float32), what + ": forward")
            same_bits(dl, gr['d_logits'].astype(np.float32), what + ": d logits")
            same_bits(df, gr['d_flow'].astype(np.float32), what + ": d flow")
        assert np.abs(fwd['out']).max() > 1 or h * w <= 5


# ---- bar 2: general logits within the derived bars -------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", uo.FACTORS)
@pytest.mark.parametrize("n,h,w", FRAMES, ids=_ids(FRAMES))
def test_general_logits_within_the_bars(n, h, w, k):
    lg, g, fwd, gr = _want("general", n, k, h, w)
    for half, masked in ((False, True), (True, False)):
        what = "%d x %d x %d k %d half %s masked %s" % (n, h, w, k, half, masked)
        out, dl, df = _run(n, k, h, w, lg, g, half, masked)
        within(out, fwd['out'], fwd['mag'], 44, what + ": forward")
        within(dl, gr['d_logits'], gr['mag_logits'], 40, what + ": d logits")
        within(df, gr['d_flow'], gr['mag_flow'], 40, what + ": d flow")
    assert np.abs(gr['d_logits']).max() > 1e-3 and np.abs(gr['d_flow']).max() > 1e-3


@gpu
@pytest.mark.parametrize("k", uo.FACTORS)
def test_one_gradient_alone_a_repeat_and_a_batch_give_the_same_bits(k):
    from oflibpytorch_amd import _native, _upsample
    n, h, w = FRAMES[-1]
    assert n == 3
    f, m = uo.case(n, h, w)
    lg, g = uo.logits_general(n, k, h, w), uo.upstream(n, k, h, w)
    v, lt, gt = _to(f), _to(lg), _to(g)
    out, om = _upsample.flow_upsample_convex(v, _to(m), lt, k)
    dl, df = _upsample.flow_upsample_convex_grad(v, lt, k, gt)
    bits = lambda t: t.view(torch.int32)
    only_l, none = _upsample.flow_upsample_convex_grad(v, lt, k, gt, want_vecs=False)
    assert none is None and torch.equal(bits(only_l), bits(dl)) and 'flow_upsample_convex_grad_logits_kernel' in _native.last_kernel_name()
    none, only_f = _upsample.flow_upsample_convex_grad(v, lt, k, gt, want_logits=False)
    assert none is None and torch.equal(bits(only_f), bits(df))
    again = _upsample.flow_upsample_convex_grad(v, lt, k, gt)
    assert torch.equal(bits(again[0]), bits(dl)) and torch.equal(bits(again[1]), bits(df))
    for b in range(n):
        o1, m1 = _upsample.flow_upsample_convex(v[b:b + 1], _to(m[b:b + 1]), lt[b:b + 1].contiguous(), k)
        assert torch.equal(bits(o1[0]), bits(out[b])) and torch.equal(m1[0], om[b])
        l1, f1 = _upsample.flow_upsample_convex_grad(v[b:b + 1], lt[b:b + 1].contiguous(), k, gt[b:b + 1].contiguous())
        assert torch.equal(bits(l1[0]), bits(dl[b])) and torch.equal(bits(f1[0]), bits(df[b]))
    # an upstream gradient that is a view at an odd offset
    odd = torch.empty(gt.numel() + 1, dtype=torch.float32, device=_dev())[1:].view_as(gt).copy_(gt)
    assert odd.data_ptr() % 16 != 0
    l2, f2 = _upsample.flow_upsample_convex_grad(v, lt, k, odd)
    assert torch.equal(bits(l2), bits(dl)) and torch.equal(bits(f2), bits(df))


# ---- bar 3: the whole API ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", uo.FACTORS)
def test_the_api_and_its_backward_against_the_oracle(k):
    import oflibpytorch_amd as ofl
    n, h, w = 2, 20, 28
    lg, g, fwd, gr = _want("general", n, k, h, w)
    f, m = uo.case(n, h, w)
    v, lt = _to(f).requires_grad_(True), _to(lg).requires_grad_(True)
    flow = ofl.Flow(v, 's', _to(m))
    up = flow.upsample_convex(lt)
    assert isinstance(up, ofl.Flow) and up.ref == 's' and up.shape == (n, k * h, k * w) and up.device == flow.device
    assert up.vecs.requires_grad and type(up.vecs.grad_fn).__name__ == "UpsampleConvexFnBackward"
    assert torch.equal(up.mask, flow.mask.repeat_interleave(k, 1).repeat_interleave(k, 2))
    what = "Flow.upsample_convex k %d" % k
    within(up.vecs.detach().cpu().numpy(), fwd['out'], fwd['mag'], 44, what + ": forward")
    up.vecs.backward(_to(g))
    within(lt.grad.cpu().numpy(), gr['d_logits'], gr['mag_logits'], 40, what + ": d logits")
    within(v.grad.cpu().numpy(), gr['d_flow'], gr['mag_flow'], 40, what + ": d flow")
    # without a gradient and without the mask: the same bits, no graph; the tensor wrapper and an fp16-stored flow likewise
    for vecs in (v.detach(), v.detach().half()):
        bare = ofl.Flow(vecs, 't', _to(m)).upsample_convex(lt.detach(), factor=k, consider_mask=False)
        assert bare.ref == 't' and not bare.vecs.requires_grad and bool(bare.mask.all())
        assert torch.equal(bare.vecs.view(torch.int32), up.vecs.detach().view(torch.int32))
    got = ofl.upsample_flow_convex(_to(f), _to(lg))
    assert got.shape == (n, 2, k * h, k * w) and torch.equal(got.view(torch.int32), up.vecs.detach().view(torch.int32))
