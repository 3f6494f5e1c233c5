"""GPU tier of Flow.from_matching on fp16 / bf16 features (ofl_matching_x16.hip) against tests/matching_x16_oracle.py:
the float64 evaluation of the definition on the exact values of the 16-bit inputs.  Both dtypes, both refs.

Frames (matching_x16_oracle.frames()), by Q = H W: 1; 1 x 5 and 5 x 1; the pixel tile (64) and the walked chunk (32), each minus one,
exact, plus one and twice plus one; a batch of 3 at 5 x 7.  Channels (channels()): 1; the K step of an MFMA (16) and twice it, each minus
one, exact and plus one; 128, the most whose fragments stay in registers, and 130, the kernel's other instantiation.

EXACT TIER, bit for bit: on features in {0, +-32} with C = 16 or 4 every logit is 0 or at most -1024, whatever the order the MFMA sums
in, exp(0) = 1 and exp(-1024) = +0, and every sum is a sum of small integers: the flow, prob and the statistics equal the float32
definition (matching_oracle.compute) on the up-converted features and the float32 route's statistics on the device byte for byte, and both
gradients are the float32 route's rounded once to the dtype.

GENERAL TIER: features N(0, 1) on a grid of 2^-6, cast (the cast to bfloat16 changes only odd multiples at |x| >= 4: asserted in the
oracle module).  The forward is held to ulp32(want) + eta A + sigma B, prob to ulp32(want) + 2 eta want, the gradients to the float32
route's bar plus half an ulp of the dtype plus the term of the statistics' deviation: matching_x16_oracle has the terms, DESIGN.md 4 the
derivation.  Every test prints the worst fraction of its bar before it asserts; a fraction above 1 means the kernel is wrong."""
import functools

import numpy as np
import pytest
import torch

import matching_oracle as mo
import matching_x16_oracle as xo

gpu = pytest.mark.gpu
FRAMES = xo.frames()
CHANNELS = xo.channels()
SIGN = {'s': -1.0, 't': 1.0}
NAMES = ('fp16', 'bf16')


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _ids(frames):
    return ["%dx%dx%d" % f for f in frames]


def _to(x):
    return torch.from_numpy(np.ascontiguousarray(x).copy()).to(_dev())


def _stats(stats, n, q):
    raw = stats.cpu().numpy()
    d = raw[:24 * n * q].view(np.float64).reshape(3, n, q)
    return raw[24 * n * q:].view(np.float32).reshape(n, q), d[0], d[1], d[2]


def _forward(ft, ot, ref):
    from oflibpytorch_amd import _matching, _native
    n, c, h, w = ft.shape
    out, prob, stats = _matching.flow_global_match_x16(ft, ot, SIGN[ref], True, True)
    name = _native.last_kernel_name()
    assert 'flow_global_match_x16_kernel' in name and ('half_t' if ft.dtype == torch.float16 else 'bf16_t') in name, name
    assert out.dtype == torch.float32 and out.shape == (n, 2, h, w) and out.is_contiguous()
    assert prob.dtype == torch.float32 and prob.shape == (n, h, w) and prob.is_contiguous()
    assert stats.dtype == torch.uint8 and stats.numel() == 28 * n * h * w
    return out, prob, stats


def _api_grads(ft, ot, gt, ref):
    """The gradients as a user gets them: Flow.from_matching on tensors that require them, in the features' dtype"""
    import oflibpytorch_amd as ofl
    f, o = ft.detach().clone().requires_grad_(True), ot.detach().clone().requires_grad_(True)
    flow = ofl.Flow.from_matching(f, o, ref)
    flow.vecs.backward(gt)
    assert f.grad.dtype == ft.dtype and o.grad.dtype == ft.dtype and f.grad.shape == ft.shape and o.grad.shape == ot.shape
    return flow.vecs.detach(), f.grad, o.grad


def _frac(got, want, bar, what):
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    frac = float((np.abs(got - want) / bar).max())
    print("%s: worst error %.4f of its bar" % (what, frac))
    assert np.isfinite(got).all(), what
    return frac


# ---- the exact tier --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,h,w", FRAMES, ids=_ids(FRAMES))
def test_exact_softmax_bit_for_bit(n, h, w):
    """Both dtypes, C = 16 and 4, every family, both refs, in one test per frame"""
    for name in NAMES:
        _exact(n, h, w, name)


def _exact(n, h, w, name):
    from oflibpytorch_amd import _matching
    bits = lambda t: t.view(torch.int16)
    gt = _to(mo.upstream(n, h, w))
    for c, kinds in ((16, ('one-hot', 'two-hot', 'all-equal', 'rising')), (4, ('one-hot', 'all-equal'))):
        for kind in kinds:
            feat, other = xo.features_exact(kind, n, c, h, w)
            (f16, fup), (o16, oup) = xo.to16(feat, xo.DTYPES[name]), xo.to16(other, xo.DTYPES[name])
            assert np.array_equal(fup, feat) and np.array_equal(oup, other)                  # both dtypes hold {0, +-32}
            ft, ot = f16.to(_dev()), o16.to(_dev())
            for ref in ('s', 't'):
                what = "%s %d x %d x %d C %d %s %s" % (name, n, h, w, c, kind, ref)
                want = mo.compute(feat, other, SIGN[ref])
                out, prob, stats = _forward(ft, ot, ref)
                assert np.array_equal(out.cpu().numpy().view(np.uint32), want['out32'].view(np.uint32)), what + ": forward"
                assert np.array_equal(prob.cpu().numpy().view(np.uint32), want['prob'].view(np.uint32)), what + ": prob"
                m, S, ox, oy = _stats(stats, n, h * w)
                assert np.array_equal(m.view(np.uint32), want['m'].view(np.uint32)) and np.array_equal(S, want['S']), what + ": m, S"
                assert np.array_equal(ox, want['ox']) and np.array_equal(oy, want['oy']), what + ": the saved expectation"
                # the float32 route on the device: the same statistics byte for byte, and its gradients rounded once
                o32, _, s32 = _matching.flow_global_match(ft.float(), ot.float(), SIGN[ref], False, True)
                assert torch.equal(s32, stats) and torch.equal(o32.view(torch.int32), out.view(torch.int32)), what + ": the float32 route"
                df, do = _matching.flow_global_match_grad(ft.float(), ot.float(), SIGN[ref], s32, gt)
                vecs, gf, go = _api_grads(ft, ot, gt, ref)
                assert torch.equal(vecs.view(torch.int32), out.view(torch.int32)), what + ": Flow.from_matching"
                assert torch.equal(bits(gf), bits(df.to(ft.dtype))), what + ": d feat"
                assert torch.equal(bits(go), bits(do.to(ft.dtype))), what + ": d other"
    if h * w == 1:
        assert not out.any() and bool((prob == 1).all())                                     # 1 x 1: the flow is exactly 0
    else:
        assert float(out.abs().max()) > 0


# ---- the general tier ------------------------------------------------------------------------------------------------------------------
_SHARED = {}


@functools.lru_cache(maxsize=None)
def _want(name, n, c, h, w):
    """The inputs and the oracle's results for an 's' flow, computed once per case and left unchanged.  A 't' flow's vectors and
    gradients are their exact negations (the sign enters as a factor of -1 alone) and its bars are the same; where the two dtypes hold
    the same values (everywhere but for the few elements the cast to bfloat16 changes) they share the float64 evaluation, and only the
    half ulp of the dtype in the gradients' bars is their own"""
    f16, o16, fup, oup = xo.features_general(name, n, c, h, w)
    g = mo.upstream(n, h, w)
    key = (n, c, h, w, fup.tobytes(), oup.tobytes())
    if key not in _SHARED:
        if len(_SHARED) >= 4:                                                                # (the other dtype of the same case comes next)
            _SHARED.clear()
        fwd = xo.compute(fup, oup, -1.0)
        _SHARED[key] = (fwd, xo.grads(fup, oup, -1.0, g, name, fwd))
    fwd, gr = _SHARED[key]
    return f16, o16, g, fwd, xo.rounded_to(gr, name)


def _general(name, n, c, h, w, ref):
    f16, o16, g, fwd, gr = _want(name, n, c, h, w)
    flip = 1.0 if ref == 's' else -1.0
    ft, ot, gt = f16.to(_dev()), o16.to(_dev()), _to(g)
    what = "%s %d x %d x %d C %d %s" % (name, n, h, w, c, ref)
    out, prob, stats = _forward(ft, ot, ref)
    fracs = [_frac(out.cpu().numpy(), flip * fwd['out'], fwd['bar'], what + ": forward"),
             _frac(prob.cpu().numpy(), fwd['want_prob'], fwd['bar_prob'], what + ": prob")]
    _, _, ox, oy = _stats(stats, n, h * w)
    saved = np.stack([ox, oy], 1).reshape(n, 2, h, w)
    fracs.append(_frac(saved, np.stack([fwd['ox'], fwd['oy']], 1).reshape(n, 2, h, w), fwd['loose'] + 2.0 ** -40, what + ": saved ox, oy"))
    _, gf, go = _api_grads(ft, ot, gt, ref)
    fracs.append(_frac(gf.float().cpu().numpy(), flip * gr['d_feat'], gr['bar_feat'], what + ": d feat"))
    fracs.append(_frac(go.float().cpu().numpy(), flip * gr['d_other'], gr['bar_other'], what + ": d other"))
    return fracs


@gpu
@pytest.mark.parametrize("n,h,w", FRAMES, ids=_ids(FRAMES))
def test_general_features_within_the_bars(n, h, w):
    """Every channel count of CHANNELS, both dtypes and both refs, in one test per frame: every case prints its fractions, and the
    test names those above 1"""
    over = []
    for c in CHANNELS:
        for name in NAMES:
            worst = np.max([_general(name, n, c, h, w, ref) for ref in ('s', 't')], 0)
            print("%s %d x %d x %d C %d: worst fractions forward %.4f prob %.4f saved %.4f d feat %.4f d other %.4f" % ((name, n, h, w, c) + tuple(worst)))
            if not (worst <= 1.0).all():
                over.append((name, c, worst.tolist()))
    assert not over, over


@gpu
def test_a_wide_frame_of_many_chunks_within_the_bars():
    """11 x 97 (Q = 1067: 17 tiles, 34 chunks and a tail of 11 positions; rows longer than a chunk), C = 24, both dtypes"""
    for name in NAMES:
        worst = _general(name, 1, 24, 11, 97, 's')
        assert max(worst) <= 1.0, (name, worst)


# ---- independence ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", [3, 130])
def test_an_image_has_the_same_bits_alone_in_a_batch_and_against_one_shared_frame(c):
    for name in NAMES:
        _independent(name, c)


def _independent(name, c):
    from oflibpytorch_amd import _matching
    n, h, w = 3, 7, 19                                                                       # Q = 133: three tiles, five chunks
    f16, o16, _, _ = xo.features_general(name, n, c, h, w)
    ft, ot = f16.to(_dev()), o16.to(_dev())
    out, prob, stats = _matching.flow_global_match_x16(ft, ot, -1.0, True, True)
    bare, none, nothing = _matching.flow_global_match_x16(ft, ot, -1.0, False, False)
    assert none is None and nothing is None and torch.equal(bare.view(torch.int32), out.view(torch.int32))
    o2, p2, s2 = _matching.flow_global_match_x16(ft, ot, -1.0, True, True)                  # a repeat
    assert torch.equal(o2.view(torch.int32), out.view(torch.int32)) and torch.equal(p2.view(torch.int32), prob.view(torch.int32))
    assert torch.equal(s2, stats)
    m, S, ox, oy = _stats(stats, n, h * w)
    for b in range(n):
        o1, p1, s1 = _matching.flow_global_match_x16(ft[b:b + 1], ot[b:b + 1], -1.0, True, True)
        assert torch.equal(o1[0].view(torch.int32), out[b].view(torch.int32)) and torch.equal(p1[0].view(torch.int32), prob[b].view(torch.int32))
        m1, S1, ox1, oy1 = _stats(s1, 1, h * w)
        assert np.array_equal(m1[0].view(np.uint32), m[b].view(np.uint32)) and np.array_equal(S1[0], S[b])
        assert np.array_equal(ox1[0], ox[b]) and np.array_equal(oy1[0], oy[b])
        o3, _, _ = _matching.flow_global_match_x16(ft[b], ot[b], -1.0)                       # C-H-W: a batch of one
        assert torch.equal(o3[0].view(torch.int32), out[b].view(torch.int32))
    # other_bs = 0: one frame of `other` for the whole batch (an `expand`ed batch is handed over as a stride of 0, not as n copies)
    shared, _, _ = _matching.flow_global_match_x16(ft, ot[1:2].expand(n, -1, -1, -1), -1.0)
    each, _, _ = _matching.flow_global_match_x16(ft, ot[1:2].expand(n, -1, -1, -1).contiguous(), -1.0)
    assert torch.equal(shared.view(torch.int32), each.view(torch.int32))
    assert torch.equal(shared[1].view(torch.int32), out[1].view(torch.int32))


# ---- the volume is never formed, and no float32 copy is kept ---------------------------------------------------------------------------
@gpu
def test_peak_memory_of_the_forward_stays_far_below_the_volume():
    """N = 2, C = 16, 40 x 48, bf16: the volume would be 14.7 MB an image in float32.  The forward's peak beyond the inputs -- the vectors,
    the packed rows, the Flow's mask -- stays under 1/16 of ONE image's volume.  A condition, not a measurement."""
    import oflibpytorch_amd as ofl
    n, c, h, w = 2, 16, 40, 48
    rng = np.random.RandomState(3)
    ft = _to(rng.normal(size=(n, c, h, w)).astype(np.float32)).bfloat16()
    ot = _to(rng.normal(size=(n, c, h, w)).astype(np.float32)).bfloat16()
    ofl.Flow.from_matching(ft, ot, 's')
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    flow = ofl.Flow.from_matching(ft, ot, 's')
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    volume = 4 * (h * w) ** 2
    print("peak beyond the inputs: %d bytes = 1 / %.1f of one image's volume of %d bytes" % (peak, volume / max(peak, 1), volume))
    assert flow.vecs.dtype == torch.float32 and peak < volume // 16
