"""GPU tier of Flow.match_local (ofl_local_match.hip) against tests/local_match_oracle.py.

Frames (local_match_oracle.frames()), every radius 1 .. 4: 2 x 2, 2 x 7, 7 x 2 and 2 x 3, smaller than the window; the width (32) and the
heights (4 of the forward, 16 of the gathers) of the tiles, each minus one, exact, plus one and twice plus one; a batch of 3; 17 x 33,
which every tile border crosses and on which the one-hot family's planted matches straddle every border in both directions (asserted).  Masks
(local_match_oracle.masks()): none; single False pixels on either side of every tile border and at the corners; a checkerboard; one
image fully False.  Both references and fp32 and fp16-stored vectors alternate over the cases of a test.

BIT FOR BIT (for any correct exp: exp(0) = 1 and exp(-1024) = +0 exactly): the forward, prob, the saved statistics, d feat and d W equal
the oracle on features in {0, +-32} with C = 16 or 4 and INTEGER vectors whose samples are values of `other` bit for bit, so that every
difference of a logit from the maximum -- the +0 of a position that is not usable included, which ties with the maximum in every family
but two-hot, whose matches lie above it and carry weights of exactly 1/2 -- is 0 or at most -1024; the upstream gradient on a grid of 2^-6.  d flow of `backward()` is, bit for bit, the upstream gradient plus the gated flow gradient of
the warp's own backward kernel run on the ORACLE's d W: the sum as defined.

GENERAL: features N(0, 1) and vectors of a few pixels on grids of 2^-6, at least a tenth of the pixels not usable.  The kernel and the
oracle take the same IEEE steps in the same order and differ in exp alone (the derivations of 3.28's local form):
  forward   held to ulp32(want) + 2^-k A against the definition before its last rounding, A = sum_o w |o - E[o]| per component,
            k = 46 - ceil(log2 T), T the participating positions of the pixel
  d feat,   held to ulp32(want) + 2^-k A against the float64 sum of the definition's float32 terms, A the sum of their absolute values,
  d W       k = 20 - ceil(log2(T + 6)), T the number of terms of the element
Every test prints the worst fraction of its bar before it asserts."""
import functools

import numpy as np
import pytest
import torch

import local_match_oracle as lo

gpu = pytest.mark.gpu
FRAMES = lo.frames()
G = lo.geometry()
GENERAL_FRAMES = [(1, 2, 3), (1, 3, G["kTileW"] + 1), (1, 2 * G["kTileH"] + 1, 5), (1, G["kGTileH"] + 1, 5), (3, 11, 13)]
RADII = lo.RADII


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _ids(frames):
    return ["%dx%dx%d" % f for f in frames]


def _to(x, half=False):
    if x is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(x).copy()).to(_dev())
    return t.half() if half else t


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
    bar = lo.ulp32(want64) + 2.0 ** -np.asarray(shift, np.float64) * mag
    err = np.abs(got.astype(np.float64) - want64)
    frac = float((err / bar).max())
    print("%s: worst error %.3f of the bar ulp32 + 2^-k A, smallest k %d" % (what, frac, int(np.min(shift))))
    assert np.isfinite(got).all() and frac <= 1.0, (what, frac)
    return frac


def stats_of(stats, n, q):
    """(m float32 [n, q]; S, ox, oy float64 [n, q]) out of the statistics"""
    raw = stats.cpu().numpy()
    d = raw[:24 * n * q].view(np.float64).reshape(3, n, q)
    return raw[24 * n * q:].view(np.float32).reshape(n, q), d[0], d[1], d[2]


@functools.lru_cache(maxsize=None)
def _want(kind, mask_name, n, c, h, w, radius, ref):
    """The inputs and the oracle's results, computed once per case and left unchanged"""
    mask, g = lo.masks(n, h, w)[mask_name], lo.upstream(n, h, w)
    if kind == "general":
        a = lo.vectors_general(n, h, w)
        feat, other = lo.features_general(n, c, h, w)
    else:
        a = lo.vectors_integer(n, h, w, ref)
        feat, other = lo.features_exact(kind, a, mask, ref, c, radius)
    fwd = lo.compute(a, mask, feat, other, ref, radius)
    return a, mask, feat, other, g, fwd, lo.grads(a, mask, feat, other, ref, radius, g, res=fwd)


def run(a, mask, feat, other, ref, radius, g, half):
    from oflibpytorch_amd import _local_match, _native
    n, c, h, w = feat.shape
    sign = lo.sign_of(ref)
    at, mt, ft, ot = _to(a, half), _to(mask), _to(feat), _to(other)
    out, prob, stats = _local_match.flow_local_match(at, mt, ft, ot, sign, radius, True, True)
    name = _native.last_kernel_name()
    assert 'flow_local_match_kernel<%d, %s, false>' % (radius, 'true' if half else 'false') in name, name
    assert out.dtype == torch.float32 and out.shape == (n, 2, h, w) and out.is_contiguous()
    assert prob.dtype == torch.float32 and prob.shape == (n, h, w)
    assert stats.dtype == torch.uint8 and stats.numel() == 28 * n * h * w
    df, dw = _local_match.flow_local_match_grad(at, mt, ft, ot, sign, radius, stats, _to(g))
    assert 'flow_local_match_gather_kernel' in _native.last_kernel_name()
    for d in (df, dw):
        assert d.dtype == torch.float32 and d.shape == (n, c, h, w) and d.is_contiguous()
    return out.cpu().numpy(), prob.cpu().numpy(), stats, df.cpu().numpy(), dw.cpu().numpy()


def _exact_cases(n, h, w, radius):
    """(c, kind, mask name, ref, fp16-stored): every family on both channel counts, every mask, both references and storages in turn"""
    names = list(lo.masks(n, h, w))
    out, i = [], 0
    for c in (16, 4):
        for kind in lo.exact_kinds(c):
            for mask_name in (names if (c, kind) == (16, 'one-hot') else (names[i % len(names)], names[(i + 1) % len(names)])):
                out.append((c, kind, mask_name, lo.REFS[i % 2], (i // 2) % 2 == 1))
                i += 1
    out.append((16, 'one-hot', 'none', lo.REFS[1], True))                                    # (the unmasked one-hot case on both references)
    return out


# ---- bar 1: bit for bit on features whose softmax is exact ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("n,h,w", FRAMES, ids=_ids(FRAMES))
def test_exact_softmax_bit_for_bit(n, h, w, radius):
    cases = _exact_cases(n, h, w, radius)
    wants = [_want(kind, mask_name, n, c, h, w, radius, ref) for c, kind, mask_name, ref, _ in cases]
    # the conditions the inputs meet, on the oracle alone, before anything runs on the device
    tie = excluded = away = moved = halves = False
    for (c, kind, mask_name, ref, _), (a, mask, feat, other, g, fwd, gr) in zip(cases, wants):
        s = fwd['s']
        d = np.where(fwd['part'], s - fwd['m'][:, None], 0)
        assert ((d == 0) | (d <= -1024)).all() and (s == np.round(s)).all()                 # every difference from the maximum
        assert set(np.unique(fwd['warped'])) <= ({0.0, 32.0} if kind == 'two-hot' else {0.0, -32.0})
        halves = halves or (kind == 'two-hot' and bool((fwd['w'] == 0.5).any()))
        un = np.stack([lo.cvo._shifted(~fwd['usable'], radius, dy, dx) for dy, dx in lo.offsets(radius)], 1)
        tie = tie or bool((un & fwd['part'] & (s == 0) & (fwd['m'][:, None] == 0)).any())
        excluded = excluded or not fwd['part'].all()
        away = away or not lo.usable_of(a, None, ref).all()
        moved = moved or (kind == 'one-hot' and np.abs(fwd['out32'] - a).max() >= 1.0)
    assert excluded and away
    if h >= 2 * radius + 3 and w >= 2 * radius + 3:
        assert tie and moved and halves
    if h > G["kGTileH"] and w > G["kGTileW"]:
        # the frame that every tile border crosses: in every one-hot case that leaves pixels usable, a planted match straddles a border of
        # the forward's tiles and of the gathers' tiles in each of the four directions
        seen = 0
        for (c, kind, mask_name, ref, _), want in zip(cases, wants):
            if kind == 'one-hot' and want[5]['usable'].any():
                for tw, th in ((G["kTileW"], G["kTileH"]), (G["kGTileW"], G["kGTileH"])):
                    cross = lo.crossings(want[5], radius, tw, th)
                    assert min(cross.values()) > 0, (c, mask_name, ref, tw, th, cross)
                seen += 1
        assert seen >= 4
    for (c, kind, mask_name, ref, half), (a, mask, feat, other, g, fwd, gr) in zip(cases, wants):
        what = "%d x %d x %d r %d C %d %s mask %s %s %s" % (n, h, w, radius, c, kind, mask_name, ref, "fp16" if half else "fp32")
        out, prob, stats, df, dw = run(a, mask, feat, other, ref, radius, g, half)
        same_bits(out, fwd['out32'], what + ": forward")
        same_bits(prob, fwd['prob'], what + ": prob")
        m, S, ox, oy = (x.reshape(n, h, w) for x in stats_of(stats, n, h * w))
        assert np.array_equal(m, fwd['m']) and np.array_equal(S, fwd['S']), what + ": the saved maximum and sum"
        assert np.array_equal(ox, fwd['ox']) and np.array_equal(oy, fwd['oy']), what + ": the saved expectation"
        same_bits(df, gr['d_feat'], what + ": d feat")
        same_bits(dw, gr['d_w'], what + ": d W")
        if kind == 'all-equal' and mask_name == 'one-image-masked':
            assert np.array_equal(S[n - 1], fwd['terms'][n - 1].astype(np.float64))        # every logit +0: the weights are 1 / T


@gpu
@pytest.mark.parametrize("ref", lo.REFS)
@pytest.mark.parametrize("radius", [1, 4])
def test_d_flow_is_the_sum_as_defined_bit_for_bit(radius, ref):
    """backward() on an exact case: d feat and d W's consequences come out of autograd; d flow equals, bit for bit, g + the gated flow
    gradient that the warp's own backward kernels give for the ORACLE's d W, and g itself where the pixel is not usable"""
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _cost_volume, _native
    n, h, w, c = 3, 11, 13, 16
    a, mask, feat, other, g, fwd, gr = _want('one-hot', 'single', n, c, h, w, radius, ref)
    at, ft, ot = (_to(x).requires_grad_(True) for x in (a, feat, other))
    mt, gt = _to(mask), _to(g)
    res = ofl.Flow(at, ref, mt).match_local(ft, ot, radius)
    same_bits(res.vecs.detach().cpu().numpy(), fwd['out32'], "forward")
    assert torch.equal(res.mask, mt)
    res.vecs.backward(gt)
    same_bits(ft.grad.cpu().numpy(), gr['d_feat'], "d feat")
    sign = lo.sign_of(ref)
    chain = _cost_volume.flow_cost_volume_chain(at.detach(), sign)
    d_other, d_warp = _native.warp_bwd_grad(chain, ot.detach(), _to(gr['d_w']), flow_sign=sign)
    d_warp = _cost_volume.flow_cost_volume_gate(at.detach(), mt, sign, d_warp)
    same_bits(ot.grad.cpu().numpy(), d_other.cpu().numpy(), "d other")
    same_bits(at.grad.cpu().numpy(), g + d_warp.cpu().numpy(), "d flow")
    un = ~np.broadcast_to(fwd['usable'][:, None], g.shape)
    assert un.any() and np.array_equal(at.grad.cpu().numpy()[un].view(np.uint32), g[un].view(np.uint32))


# ---- bar 2: general features within the derived bars -----------------------------------------------------------------------------------
def _general(n, h, w, c, radius, cases):
    worst = {}
    for mask_name, ref, half in cases:
        a, mask, feat, other, g, fwd, gr = _want("general", mask_name, n, c, h, w, radius, ref)
        assert (~fwd['usable']).mean() >= 0.1
        what = "%d x %d x %d r %d C %d mask %s %s %s" % (n, h, w, radius, c, mask_name, ref, "fp16" if half else "fp32")
        out, prob, _, df, dw = run(a, mask, feat, other, ref, radius, g, half)
        fr = {'forward': within(out, fwd['out'], fwd['mag'], lo.forward_shift(fwd['terms'])[:, None], what + ": forward")}
        for name, got in (('d_feat', df), ('d_w', dw)):
            fr[name] = within(got, gr[name + '64'], gr['mag_' + name], lo.grad_shift(gr['terms_' + name]), what + ": " + name)
        assert np.abs(prob.astype(np.float64) - 1.0 / fwd['S']).max() <= 2.0 ** -22
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in fr.items()}
    return worst


@gpu
@pytest.mark.parametrize("c", [1, 5, 16])
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("n,h,w", GENERAL_FRAMES, ids=_ids(GENERAL_FRAMES))
def test_general_features_within_the_bars(n, h, w, radius, c):
    _general(n, h, w, c, radius, (('none', 's', False), ('checker', 't', True), ('single', 't', False), ('one-image-masked', 's', True)))


@gpu
@pytest.mark.parametrize("c", lo.channels())
def test_channel_chunks_within_the_bars(c):
    """C = 1 and around the channel chunk, and two chunks plus one, on a frame of two tiles plus one in both directions of the forward's
    tile (9 x 33), r = 2 and r = 4"""
    _general(1, 2 * G["kTileH"] + 1, G["kTileW"] + 1, c, 2, (('checker', 's', False),))
    _general(1, 2 * G["kTileH"] + 1, G["kTileW"] + 1, c, 4, (('single', 't', True),))


@gpu
def test_one_gradient_alone_a_repeat_and_a_batch_give_the_same_bits():
    from oflibpytorch_amd import _local_match
    n, h, w, c, radius = 3, 11, 13, 5, 2
    a, mask, feat, other, g, _, _ = _want("general", "checker", n, c, h, w, radius, 't')
    at, mt, ft, ot, gt = _to(a), _to(mask), _to(feat), _to(other), _to(g)
    bits = lambda t: t.view(torch.int32)
    fwd, bwd = _local_match.flow_local_match, _local_match.flow_local_match_grad
    out, prob, stats = fwd(at, mt, ft, ot, 1.0, radius, True, True)
    grads = bwd(at, mt, ft, ot, 1.0, radius, stats, gt)
    bare, no_prob, nothing = fwd(at, mt, ft, ot, 1.0, radius, False, False)
    assert no_prob is None and nothing is None and torch.equal(bits(bare), bits(out))
    for i in range(2):
        wants = [j == i for j in range(2)]
        only = bwd(at, mt, ft, ot, 1.0, radius, stats, gt, *wants)
        assert [o is not None for o in only] == wants and torch.equal(bits(only[i]), bits(grads[i]))
    o2, p2, s2 = fwd(at, mt, ft, ot, 1.0, radius, True, True)
    assert torch.equal(bits(o2), bits(out)) and torch.equal(bits(p2), bits(prob)) and torch.equal(s2, stats)
    for b in range(n):
        one = lambda t: t[b:b + 1].contiguous()
        o1, _, s1 = fwd(one(at), one(mt), one(ft), one(ot), 1.0, radius, False, True)
        assert torch.equal(bits(o1[0]), bits(out[b]))
        g1 = bwd(one(at), one(mt), one(ft), one(ot), 1.0, radius, s1, one(gt))
        assert all(torch.equal(bits(x[0]), bits(y[b])) for x, y in zip(g1, grads))
        o3, _, _ = fwd(one(at), one(mt), ft[b], ot[b], 1.0, radius, False, False)              # C-H-W operands
        assert torch.equal(bits(o3[0]), bits(out[b]))


# ---- bar 3: the autograd route -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("chw", [False, True])
@pytest.mark.parametrize("ref", lo.REFS)
@pytest.mark.parametrize("radius,c", [(4, 5), (1, 3)])
def test_backward_against_float64_autograd_of_the_definition(radius, c, ref, chw):
    """20 x 28: d feat, d other and d flow of backward() against torch's float64 autograd of the definition (local_match_oracle.textbook)
    within 2e-4 of each gradient's scale, the bar tests/test_gpu_cost_volume.py holds the same warp-backward kernels to;
    d flow is g bit for bit where the pixel is not usable"""
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _native
    n, h, w = 2, 20, 28
    feat, other = lo.features_general(n, c, h, w)
    if chw:
        feat, other = feat[0], other[0]
    a, g, mask = lo.vectors_general(n, h, w), lo.upstream(n, h, w), lo.masks(n, h, w)['checker']
    usable = lo.usable_of(a, mask, ref)
    want = lo.textbook(a, usable, feat, other, ref, radius, g)
    at, ft, ot = (_to(x).requires_grad_(True) for x in (a, feat, other))
    mt, gt = _to(mask), _to(g)
    res = ofl.Flow(at, ref, mt).match_local(ft, ot, radius)
    assert res.vecs.requires_grad and type(res.vecs.grad_fn).__name__ == "LocalMatchFnBackward"
    assert np.abs(res.vecs.detach().cpu().numpy() - want['out']).max() <= 1e-4 * np.abs(want['out']).max()
    res.vecs.backward(gt)
    assert 'flow_cost_volume_gate_kernel' in _native.last_kernel_name()
    for name, t, ref64 in (("feat", ft, want['d_feat']), ("other", ot, want['d_other']), ("flow", at, want['d_flow'])):
        got = t.grad.cpu().numpy()
        assert got.shape == ref64.shape == tuple(t.shape), name                              # a C-H-W operand gets a C-H-W gradient
        err, scale = np.abs(got - ref64).max(), np.abs(ref64).max()
        print("r %d C %d %s %s d %s: %.3e of the scale (bar 2e-4)" % (radius, c, ref, "C-H-W" if chw else "N-C-H-W", name, err / scale))
        assert scale > 0 and err <= 2e-4 * scale, name
    un = ~np.broadcast_to(usable[:, None], g.shape)
    assert un.any() and np.array_equal(at.grad.cpu().numpy()[un].view(np.uint32), g[un].view(np.uint32))
    # detached vectors: no launch of the warp's backward for the flow and no gate; without `other` either, no chain and no warp backward
    from oflibpytorch_amd import _cost_volume
    calls = []
    real = {"warp": _native.warp_bwd_grad, "chain": _cost_volume.flow_cost_volume_chain, "gate": _cost_volume.flow_cost_volume_gate}

    def spy(name):
        def run(*args, **kw):
            calls.append((name, kw.get("want_src"), kw.get("want_flow")))
            return real[name](*args, **kw)
        return run
    _native.warp_bwd_grad, _cost_volume.flow_cost_volume_chain, _cost_volume.flow_cost_volume_gate = spy("warp"), spy("chain"), spy("gate")
    try:
        f2, o2 = ft.detach().clone().requires_grad_(True), ot.detach().clone().requires_grad_(True)
        ofl.Flow(at.detach(), ref, mt).match_local(f2, o2, radius).vecs.backward(gt)
        assert calls == [("chain", None, None), ("warp", True, False)], calls
        del calls[:]
        f3 = ft.detach().clone().requires_grad_(True)
        ofl.Flow(at.detach(), ref, mt).match_local(f3, ot.detach(), radius).vecs.backward(gt)
        assert calls == [] and 'flow_local_match_gather_kernel' in _native.last_kernel_name()
    finally:
        _native.warp_bwd_grad, _cost_volume.flow_cost_volume_chain, _cost_volume.flow_cost_volume_gate = real["warp"], real["chain"], real["gate"]
    assert torch.equal(f2.grad.view(torch.int32), ft.grad.view(torch.int32)) and torch.equal(o2.grad.view(torch.int32), ot.grad.view(torch.int32))
    assert torch.equal(f3.grad.view(torch.int32), ft.grad.view(torch.int32))


# ---- bar 4: a planted case through Flow.match_local --------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ref", lo.REFS)
def test_a_planted_shift_is_found_exactly(ref):
    """17 x 33, one-hot code features (the class of a pixel is its position modulo 5 in both directions): `other` is `feat` shifted by
    (2, -1), the flow is (1, 0) off that shift everywhere, r = 2.  Every pixel whose match is in the frame gets exactly the shift, with
    prob 1; the returned mask is the flow's own."""
    import oflibpytorch_amd as ofl
    h, w, r = 17, 33, 2
    yy, xx = np.mgrid[0:h, 0:w]
    onehot = lambda cls: (32.0 * (cls[None] == np.arange(25)[:, None, None])).astype(np.float32)
    feat = onehot((yy % 5) * 5 + xx % 5)
    other = onehot(((yy + 1) % 5) * 5 + (xx - 2) % 5)                                         # other(q) = feat(q - (2, -1))
    sign = lo.sign_of(ref)
    shift = np.array([2.0, -1.0], np.float32) * -sign                                        # the vector that points at the match
    start = shift - np.array([1.0, 0.0], np.float32) * -sign
    a = np.broadcast_to(start[None, :, None, None], (1, 2, h, w)).copy()
    mask = lo.masks(1, h, w)['checker']
    flow = ofl.Flow(_to(a), ref, _to(mask))
    res, prob = flow.match_local(_to(feat), _to(other), r, consider_mask=False, return_prob=True)
    assert torch.equal(res.mask, flow.mask) and res.ref == ref
    found = (xx + 1 < w) & (xx + 2 < w) & (yy - 1 >= 0)                                       # p + (1, 0) is in the frame and samples inside it
    got = res.vecs.cpu().numpy()[0]
    assert found.sum() > h * w // 2
    assert (got[0][found] == shift[0]).all() and (got[1][found] == shift[1]).all()
    assert (prob.cpu().numpy()[0][found] == 1.0).all()
