"""GPU tier of Flow.corr_lookup (ofl_corr_lookup.hip) against tests/corr_lookup_oracle.py.  Every step of the
definition is a single IEEE operation in a fixed order, so the lookup, d feat and every d other_l are the oracle's BIT FOR BIT (the bits
of a NaN's payload exempt).  The whole API -- a single `other` tensor pooled by torch, autograd through the pooling -- is held to the
float64 autograd of RAFT's all-pairs expression within the bar of DESIGN.md 4 for gradient kernels, 2e-4 of the gradient's scale.

Frames (corr_lookup_oracle.frames()): 20 x 28; the kernel's 32 x 8 tile minus one, itself, plus one and two tiles plus one in both axes;
3 x 3 (smaller than every window); a batch of 3.  Explicit level tensors (level_sizes()): H x W, H/2 x W/2, 1 x 1 and (H + 3) x (W - 5)
at l = 0 .. 3.  Channel counts (channel_counts()): 1, a chunk of the d other gather minus one, the chunk, plus one, two chunks and three.
The forward has ONE route (direct global loads of the nodes), so there is no route to name beyond the kernel."""
import functools

import numpy as np
import pytest
import torch

import corr_lookup_oracle as cl

gpu = pytest.mark.gpu
FRAMES = cl.frames()
TABLE = FRAMES[0]                                    # (2, 20, 28)


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _ids(frames):
    return ["%dx%dx%d" % f for f in frames]


def _to(x):
    if isinstance(x, (list, tuple)):
        return [_to(y) for y in x]
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x).copy()).to(_dev())


@functools.lru_cache(maxsize=None)
def _vecs(n, h, w, ref, half):
    a = cl.case(n, h, w, ref)[0]
    a = a.astype(np.float16) if half else a
    a.setflags(write=False)
    return a


def _operands(n, c, h, w, ref, masked=True, half=False, chw=False):
    """(a, mask or None, feat, [levels]) as arrays"""
    feat, lv = cl.explicit_levels(n, c, h, w, ref)
    if chw:
        feat, lv = feat[0], [x[n - 1] for x in lv]
    return _vecs(n, h, w, ref, half), (cl.case(n, h, w, ref)[1] if masked else None), feat, lv


def same_bits(got, want, what):
    """Equal bit for bit; where both are NaN the payload is exempt"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        at = tuple(int(i[0]) for i in np.nonzero(bad))
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, expected %r" % (what, int(bad.sum()), bad.size, at,
                                                                                                 got[at], want[at]))


def _lookup(ops, ref, radius):
    from oflibpytorch_amd import _corr_lookup
    a, m, feat, lv = ops
    return _corr_lookup.flow_corr_lookup(_to(a), _to(m), _to(feat), _to(lv), cl.sign_of(ref), radius)


def _grads(ops, ref, radius, g, **kw):
    from oflibpytorch_amd import _corr_lookup
    a, m, feat, lv = ops
    return _corr_lookup.flow_corr_lookup_grad(_to(a), _to(m), _to(feat), _to(lv), cl.sign_of(ref), radius, _to(g), **kw)


def _configs(n, h, w):
    """(masked, half, radius, channels, chw) of a frame"""
    if (n, h, w) == TABLE:
        return [(True, False, r, 3, False) for r in cl.RADII] + [(True, False, 4, c, False) for c in cl.channel_counts()] + \
               [(True, True, 4, 5, False), (False, True, 2, 2, False), (True, False, 3, 6, True), (False, False, 1, 17, True)]
    return [(True, False, 4, 3, False), (False, True, 1, 10, False)]


# ---- bar 1: the lookup --------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,h,w", FRAMES, ids=_ids(FRAMES))
def test_lookup_against_the_oracle(n, h, w):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _native
    for ref in cl.REFS:
        for masked, half, radius, c, chw in _configs(n, h, w):
            ops = _operands(n, c, h, w, ref, masked, half, chw)
            what = "%d x %d '%s' masked %s half %s radius %d C %d chw %s" % (h, w, ref, masked, half, radius, c, chw)
            want = cl.compute(*ops, ref, radius)['lookup']
            out = _lookup(ops, ref, radius)
            assert 'flow_corr_lookup_kernel' in _native.last_kernel_name()
            assert out.dtype == torch.float32 and out.shape == (n, 4 * (2 * radius + 1) ** 2, h, w) and out.is_contiguous(), what
            same_bits(out.cpu().numpy(), want, what)
            # the API with a sequence of levels: the same bits
            a, m, feat, lv = ops
            flow = ofl.Flow(_to(a), ref, _to(cl.case(n, h, w, ref)[1]))
            got = flow.corr_lookup(_to(feat), _to(lv), radius=radius, consider_mask=masked)
            assert not got.requires_grad
            same_bits(got.cpu().numpy(), want, what + " (Flow.corr_lookup)")
        assert np.abs(want).max() > 1e-3


# ---- bar 2: d feat and d other ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,h,w", FRAMES, ids=_ids(FRAMES))
def test_gradients_against_the_oracle(n, h, w):
    from oflibpytorch_amd import _native
    k = cl.geometry()["kChanChunk"]
    configs = [(True, False, 4, c, False) for c in cl.channel_counts()] + [(True, False, 1, 3, False), (False, True, 2, 2, True),
                                                                            (True, True, 3, 2, False)]
    if (n, h, w) != TABLE:
        configs = [(True, False, 4, k + 1, False), (False, True, 1, 3, True)]
    for ref in cl.REFS:
        for masked, half, radius, c, chw in configs:
            ops = _operands(n, c, h, w, ref, masked, half, chw)
            what = "%d x %d '%s' masked %s half %s radius %d C %d chw %s" % (h, w, ref, masked, half, radius, c, chw)
            g = cl.upstream(n, 4 * (2 * radius + 1) ** 2, h, w)
            want_f, want_l = cl.grads(*ops, ref, radius, g)
            d_feat, d_levels = _grads(ops, ref, radius, g)
            assert 'flow_corr_lookup_grad_other_kernel' in _native.last_kernel_name()
            assert d_feat.dtype == torch.float32 and d_feat.shape == (n, c, h, w) and d_feat.is_contiguous(), what
            same_bits(d_feat.cpu().numpy(), want_f, what + ": d feat")
            for l, ((hl, wl), got, want) in enumerate(zip(cl.level_sizes(h, w), d_levels, want_l)):
                assert got.dtype == torch.float32 and got.shape == (n, c, hl, wl) and got.is_contiguous(), what
                same_bits(got.cpu().numpy(), want, what + ": d other %d" % l)
        # one output alone: the same bits, the others not made
        only_f, none = _grads(ops, ref, radius, g, want_levels=[False] * 4)
        assert none == [None] * 4 and torch.equal(only_f, d_feat) and 'flow_corr_lookup_grad_feat_kernel' in _native.last_kernel_name()
        none, only_2 = _grads(ops, ref, radius, g, want_feat=False, want_levels=[False, False, True, False])
        assert none is None and [x is None for x in only_2] == [True, True, False, True] and torch.equal(only_2[2], d_levels[2])
        assert np.abs(want_f).max() > 1e-3 and np.abs(want_l[0]).max() > 1e-3


@gpu
def test_a_batch_gives_the_bits_of_its_images_run_singly_and_a_repeat_the_same_bits():
    n, h, w = FRAMES[-1]
    assert n == 3
    for ref, radius, c in (('s', 4, cl.channel_counts()[3]), ('t', 2, 3)):
        a, m, feat, lv = _operands(n, c, h, w, ref)
        g = cl.upstream(n, 4 * (2 * radius + 1) ** 2, h, w)
        batch = _lookup((a, m, feat, lv), ref, radius).cpu().numpy()
        b_feat, b_lv = _grads((a, m, feat, lv), ref, radius, g)
        r_feat, r_lv = _grads((a, m, feat, lv), ref, radius, g)                               # a repeat run: identical bits
        assert torch.equal(b_feat.view(torch.int32), r_feat.view(torch.int32))
        for x, y in zip(b_lv, r_lv):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
        for i in range(n):
            one = (a[i:i + 1], m[i:i + 1], feat[i:i + 1], [x[i:i + 1] for x in lv])
            same_bits(_lookup(one, ref, radius).cpu().numpy()[0], batch[i], "image %d alone against the batch" % i)
            o_feat, o_lv = _grads(one, ref, radius, g[i:i + 1])
            same_bits(o_feat.cpu().numpy()[0], b_feat.cpu().numpy()[i], "d feat of image %d alone" % i)
            for l in range(4):
                same_bits(o_lv[l].cpu().numpy()[0], b_lv[l].cpu().numpy()[i], "d other %d of image %d alone" % (l, i))


@gpu
@pytest.mark.parametrize("ref", cl.REFS)
def test_a_smooth_flow(ref):
    """Neighbouring windows overlap: the lists of the d other gather hold few pixels each and every cell is hit"""
    n, c, h, w, radius = 1, 9, 17, 33, 4
    a, m = cl.smooth_case(n, h, w, ref)
    feat, lv = cl.explicit_levels(n, c, h, w, ref)
    g = cl.upstream(n, 4 * 81, h, w)
    same_bits(_lookup((a, m, feat, lv), ref, radius).cpu().numpy(), cl.compute(a, m, feat, lv, ref, radius)['lookup'], "the smooth flow")
    want_f, want_l = cl.grads(a, m, feat, lv, ref, radius, g)
    d_feat, d_levels = _grads((a, m, feat, lv), ref, radius, g)
    same_bits(d_feat.cpu().numpy(), want_f, "d feat")
    for l in range(4):
        same_bits(d_levels[l].cpu().numpy(), want_l[l], "d other %d" % l)


# ---- bar 3: the whole API with a single `other` tensor ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("chw", [False, True], ids=["nchw", "chw"])
@pytest.mark.parametrize("ref", cl.REFS)
def test_the_api_with_one_tensor_and_its_backward_against_the_float64_reference(ref, chw):
    import oflibpytorch_amd as ofl
    n, h, w = TABLE
    for radius, levels, c, masked in ((4, 4, 5, True), (1, 3, 3, False)):
        a, m = cl.case(n, h, w, ref)
        feat, other = cl.features(n, c, h, w, ref), cl.features(n, c, h, w, ref, salt=1)
        if chw:
            feat, other = feat[0], other[n - 1]
        d = (2 * radius + 1) ** 2
        g = cl.upstream(n, levels * d, h, w)
        ft, ot = (_to(x).requires_grad_(True) for x in (feat, other))
        flow = ofl.Flow(_to(a), ref, _to(m))
        out = flow.corr_lookup(ft, ot, radius=radius, levels=levels, consider_mask=masked)
        assert out.requires_grad and type(out.grad_fn).__name__ == "CorrLookupFnBackward" and out.shape == (n, levels * d, h, w)
        # the same bits as per-level calls on avg_pool2d outputs
        pyr = ofl.corr_pyramid(_to(other), levels)
        for l, lv in enumerate(pyr):
            one = _lookup((a, m if masked else None, feat, [np.zeros((c, 1, 1), np.float32)] * l + [lv.cpu().numpy()]), ref, radius)
            same_bits(out.detach().cpu().numpy()[:, l * d:(l + 1) * d], one.cpu().numpy()[:, l * d:], "level %d alone" % l)
        same_bits(out.detach().cpu().numpy(), cl.compute(a, m if masked else None, feat, [x.cpu().numpy() for x in pyr], ref, radius)['lookup'],
                  "the forward of the autograd route")
        out.backward(_to(g))
        want = cl.torch_reference(a, m if masked else None, feat, other, ref, radius, levels=levels, g=g)
        assert np.abs(out.detach().cpu().numpy() - want['lookup']).max() <= 1e-5 * np.abs(want['lookup']).max()
        for name, got, ref64 in (("feat", ft.grad, want['d_feat']), ("other", ot.grad, want['d_other'])):
            got = got.cpu().numpy()
            scale = np.abs(ref64).max()
            err = np.abs(got - ref64).max()
            print("'%s' radius %d chw %s d %s: max error %.3e of a scale %.3e" % (ref, radius, chw, name, err, scale))
            assert got.dtype == np.float32 and got.shape == ref64.shape and scale > 1e-2, name
            assert err <= 2e-4 * scale, name
