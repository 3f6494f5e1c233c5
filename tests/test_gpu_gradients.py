"""GPU tier: the backward passes and the side kernels of ofl_aux_kernels.hip at the shapes and edges where their code branches,
against tests/grad_ref.py (the reference's op sequences restated with torch ops, autograd on the CPU; pinned to the
reference's fixtures by tests/test_grad_ref_golden.py) and against the CPU oracle.

  a. gradients of the composed operations (switch_ref, invert, combine_with 1 / 2 / 3, Flow.apply to a Flow, Flow.combine,
     padded apply) on staged-kernel sizes, with exactly-zero vectors (occlusion rule, un-occlude fill), taps that leave the
     frame, masks with holes and batch broadcasts;
  b. frames of width 2 and 3: the gradient wrt the warped image on the float-atomics warp_grad_kernel;
  c. track_pts / Flow.track (sample_pts_kernel<false / true>): edges of the frame, integer points, broadcasts, 20 000 points
     in one cell;
  d. get_padding (flow_extents_kernel): the grid-stride reduction at 1080p, thresholds, -0.0, single valid pixels.

Bars: gradients within case_runner.GRAD_RTOL of the gradient's scale (5e-4 for positions), masks and padding exactly, the
forward of the samplers and reductions bit for bit.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import case_runner
import grad_ref
from grad_ref import RFlow

pytestmark = pytest.mark.gpu

POS_RTOL = 5e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tier needs a HIP device"
    from oflibpytorch_amd import _native
    _native.load_library()
    return torch.device('cuda', 0)


def _close(got, exp, what, rtol=case_runner.GRAD_RTOL):
    assert got is not None, "%s: no gradient" % what
    got = got.detach().cpu()
    assert got.shape == exp.shape, "%s: shape %s != %s" % (what, tuple(got.shape), tuple(exp.shape))
    scale = float(exp.abs().max())
    err = float((got.double() - exp.double()).abs().max())
    assert err <= rtol * max(scale, 1e-6), "%s: max |diff| %.3g against a scale of %.3g" % (what, err, scale)


def _smooth(n, h, w, sigma, seed):
    g = torch.Generator().manual_seed(seed)
    lo = torch.randn(n, 2, max(h // 12, 2), max(w // 12, 2), generator=g) * sigma
    return F.interpolate(lo, size=(h, w), mode='bicubic', align_corners=True).contiguous()


def _field(n, h, w, sigma, seed, shift=True):
    """A smooth flow, exactly zero in a disc of every image but the first (the envelope ramps up over 8 px: no folds), the
    first image shifted so that taps and end points leave the frame."""
    f = _smooth(n, h, w, sigma, seed)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    r = max(min(h, w) // 8, 2)
    env = torch.clamp((torch.sqrt((ys - h / 3) ** 2 + (xs - w / 2) ** 2) - r) / 8.0, 0.0, 1.0)
    k0 = 1 if (shift and n > 1) else 0
    f[k0:] = f[k0:] * env
    if shift:
        f[0] += torch.tensor([0.15 * w, -0.1 * h]).view(2, 1, 1)
    return f.contiguous()


def _holes(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(n, h, w, generator=g) > 0.1
    m[:, h // 2:h // 2 + max(h // 6, 1), w // 5:w // 5 + max(w // 6, 1)] = False
    return m


def _kernel():
    from oflibpytorch_amd import _native
    return _native.last_kernel_name()


# ------------------------------------------------------------------------------------------------
# a. composed operations
# ------------------------------------------------------------------------------------------------
def _run_flow_op(op, fl_cls, fa, fb, ref, ma, mb):
    a, b = fl_cls(fa, ref, ma), fl_cls(fb, ref, mb)
    other = 't' if ref == 's' else 's'
    if op == 'switch_ref':
        return a.switch_ref()
    if op == 'invert':
        return a.invert()
    if op == 'invert_other':
        return a.invert(other)
    if op.startswith('combine_with'):
        return a.combine_with(b, int(op[-1]))
    if op == 'apply_flow':
        return a.apply(fl_cls(fb, other, mb))
    if op == 'apply_flow_bcast':                       # a batch-1 flow applied to a batch-N flow
        return fl_cls(fa[:1], ref, ma[:1]).apply(fl_cls(fb, other, mb))
    if op.startswith('combine_'):                      # combine_<mode><self ref><other ref><out ref>
        m, sr, orf, outr = int(op[8]), op[9], op[10], op[11]
        return fl_cls(fa, sr, ma).combine(fl_cls(fb, orf, mb), m, outr)
    raise KeyError(op)


# one Flow.combine cell per plan kind (switch of the far field yes / no x carried back and added / added and carried forward)
COMBINE_CELLS = ['combine_3stt', 'combine_1tst', 'combine_1tss', 'combine_2sst']
FLOW_OPS = ['switch_ref', 'invert', 'invert_other', 'combine_with1', 'combine_with2', 'combine_with3', 'apply_flow',
            'apply_flow_bcast']


def _compare_flow_op(op, ref, n, h, w, dev, seed=0):
    fa0 = _field(n, h, w, 3.0, 11 + seed)
    fb0 = _field(n, h, w, 2.5, 12 + seed, shift=False)
    ma, mb = _holes(n, h, w, 2 + seed), _holes(n, h, w, 3 + seed)
    wts = torch.randn(n, 2, h, w, generator=torch.Generator().manual_seed(5 + seed))
    import oflibpytorch_amd as ofl
    fa, fb = fa0.to(dev).requires_grad_(), fb0.to(dev).requires_grad_()
    out = _run_flow_op(op, ofl.Flow, fa, fb, ref, ma.to(dev), mb.to(dev))
    kernel = _kernel()
    assert out.vecs.grad_fn is not None
    (out.vecs * wts.to(dev)).sum().backward()
    ca, cb = fa0.clone().requires_grad_(), fb0.clone().requires_grad_()
    exp = _run_flow_op(op, RFlow, ca, cb, ref, ma, mb)
    assert out.ref == exp.ref
    assert torch.equal(out.mask.cpu(), exp.mask), "%s: %d mask bits differ" % (op, int((out.mask.cpu() != exp.mask).sum()))
    _close(out.vecs, exp.vecs.detach(), "%s %s: vecs" % (op, ref))
    (exp.vecs * wts).sum().backward()
    for what, got, e in (("grad wrt self", fa.grad, ca.grad), ("grad wrt other", fb.grad, cb.grad)):
        if e is None:
            assert got is None or not bool(got.any()), "%s %s: %s should be zero" % (op, ref, what)
        else:
            _close(got, e, "%s %s: %s" % (op, ref, what), rtol=POS_RTOL)
    return kernel


STAGED_SHAPES = [(3, 96, 136), (2, 270, 480)]


@pytest.mark.parametrize("shape", STAGED_SHAPES)
@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("op", FLOW_OPS)
def test_composed_operation_gradients(op, ref, shape, dev):
    """WarpFn / SplatFn backward chains (ofl_warp_bwd_grad_f32: staged column / row kernels or warp_grad_kernel; ofl_splat_grad_f32:
    splat_grad_prep_kernel + splat_grad_kernel; ofl_splat_sum_f32 for the gradient wrt a warped field), through the fused
    epilogues of combine (addend aliasing the flow in mode 3, the `src_b` difference of modes 1 / 2) and `_reduce_to` for the
    batch-1 flow.  Flows with exactly-zero discs (occlusion rule and un-occlude fill of every 's' splat), taps that leave the
    frame, masks with holes."""
    n, h, w = shape
    kernel = _compare_flow_op(op, ref, n, h, w, dev)
    if op == 'combine_with3' and ref == 't':
        # mode 3 't' is ONE fused gather on the staged kernels at these sizes
        assert "rows_kernel" in kernel or "column_kernel" in kernel, kernel


@pytest.mark.parametrize("shape", STAGED_SHAPES)
@pytest.mark.parametrize("op", COMBINE_CELLS)
def test_combine_cell_gradients(op, shape, dev):
    """Flow.combine, one (mode, self ref, other ref, out ref) cell per plan kind: `_carry_back_and_add` (the fused gather with
    the addend) and `_add_and_carry_forward` (the splat of a sum or of a `data - data_b` difference), with and without the
    switch_ref of the far field."""
    n, h, w = shape
    _compare_flow_op(op, 's', n, h, w, dev)


@pytest.mark.parametrize("case", [('combine_with3', 't'), ('combine_with1', 's')])
def test_composed_operation_gradients_1080p(case, dev):
    """Mode 3 't' (fused gather with the addend aliasing the flow, the row-table kernels at B = 1 1080p) and mode 1 's' (two
    splats and a warp: the `src_b` difference and the splat backward with zero vectors) on one 1080p frame."""
    op, ref = case
    kernel = _compare_flow_op(op, ref, 1, 1080, 1920, dev, seed=7)
    if op == 'combine_with3':
        assert "rows_kernel" in kernel or "column_kernel" in kernel, kernel


@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("cut", [True, False])
def test_padded_apply_gradients(ref, cut, dev):
    """Flow.apply(padding=..., cut=...) with gradients: the padded-copy route (Flow.pad, then apply_flow), gradients wrt the flow
    (through F.pad's replicate / constant border) and the larger target, valid area exactly."""
    import oflibpytorch_amd as ofl
    n, h, w = 2, 64, 90
    pad = [5, 3, 7, 2]
    f0 = _field(n, h, w, 3.0, 31)
    m = _holes(n, h, w, 32)
    g = torch.Generator().manual_seed(33)
    img0 = torch.rand(n, 3, h + pad[0] + pad[1], w + pad[2] + pad[3], generator=g)
    oh, ow = (h, w) if cut else img0.shape[-2:]
    wts = torch.randn(n, 3, oh, ow, generator=g)
    fa, ia = f0.to(dev).requires_grad_(), img0.to(dev).requires_grad_()
    out, valid = ofl.Flow(fa, ref, m.to(dev)).apply(ia, return_valid_area=True, padding=pad, cut=cut)
    (out * wts.to(dev)).sum().backward()
    fb, ib = f0.clone().requires_grad_(), img0.clone().requires_grad_()
    eo, ev = RFlow(fb, ref, m).apply(ib, return_valid_area=True, padding=pad, cut=cut)
    (eo * wts).sum().backward()
    assert torch.equal(valid.cpu(), ev)
    _close(out, eo.detach(), "padded apply %s cut=%s: out" % (ref, cut))
    _close(fa.grad, fb.grad, "padded apply %s cut=%s: grad wrt flow" % (ref, cut), rtol=POS_RTOL)
    _close(ia.grad, ib.grad, "padded apply %s cut=%s: grad wrt target" % (ref, cut))


@pytest.mark.parametrize("ref", ['s', 't'])
def test_batch_one_target_gradients(ref, dev):
    """A batch-1 image warped by N flows: the gradient wrt the image is the sum over the batch (`_reduce_to`, and the broadcast
    source of ofl_warp_bwd_grad_f32 / ofl_splat_grad_f32)."""
    import oflibpytorch_amd as ofl
    n, h, w = 3, 96, 136
    f0, m = _field(n, h, w, 3.0, 41), _holes(n, h, w, 42)
    g = torch.Generator().manual_seed(43)
    img0 = torch.rand(1, 3, h, w, generator=g)
    wts = torch.randn(n, 3, h, w, generator=g)
    fa, ia = f0.to(dev).requires_grad_(), img0.to(dev).requires_grad_()
    (ofl.Flow(fa, ref, m.to(dev)).apply(ia) * wts.to(dev)).sum().backward()
    fb, ib = f0.clone().requires_grad_(), img0.clone().requires_grad_()
    (RFlow(fb, ref, m).apply(ib) * wts).sum().backward()
    assert ia.grad.shape == img0.shape
    _close(ia.grad, ib.grad, "batch-1 target %s: grad wrt target" % ref)
    _close(fa.grad, fb.grad, "batch-1 target %s: grad wrt flow" % ref, rtol=POS_RTOL)


@pytest.mark.parametrize("ref", ['s', 't'])
def test_batch_one_flow_gradients(ref, dev):
    """apply_flow with ONE flow over a batch of N images (utils.py:532-537 expands the flow): the gradient wrt the flow is the sum of
    the N images' gradients (`_reduce_to` of a broadcast operand)."""
    import oflibpytorch_amd as ofl
    n, h, w = 3, 96, 136
    f0, m = _field(1, h, w, 3.0, 45, shift=False), _holes(1, h, w, 46)
    g = torch.Generator().manual_seed(47)
    img0 = torch.rand(n, 3, h, w, generator=g)
    wts = torch.randn(n, 3, h, w, generator=g)
    fa, ia = f0.to(dev).requires_grad_(), img0.to(dev).requires_grad_()
    (ofl.apply_flow(fa, ia, ref, m.to(dev)) * wts.to(dev)).sum().backward()
    fb, ib = f0.clone().requires_grad_(), img0.clone().requires_grad_()
    (grad_ref.apply_flow(fb, ib, ref, m) * wts).sum().backward()
    assert fa.grad.shape == f0.shape
    _close(fa.grad, fb.grad, "batch-1 flow %s: grad wrt flow" % ref, rtol=POS_RTOL)
    _close(ia.grad, ib.grad, "batch-1 flow %s: grad wrt target" % ref)


# ------------------------------------------------------------------------------------------------
# b. frames of width 2 and 3: the float-atomics warp_grad_kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 5, 2), (3, 2, 7, 3), (2, 4, 6, 3)])
@pytest.mark.parametrize("bcast", [False, True])
@pytest.mark.parametrize("op", ['apply_t', 'apply_s', 'mode3_t', 'mode3_s'])
def test_narrow_frame_gradients_on_the_atomics_kernel(op, bcast, shape, dev):
    """W < 4: `splat_sum` declines the frame, so the gradient wrt the warped image runs on warp_grad_kernel's float atomics
    (four taps per pixel and channel; with a batch-1 image, the atomics of N images land in one).  Apply 't' / 's' and mode 3
    against grad_ref."""
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _native
    n, c, h, w = shape
    g = torch.Generator().manual_seed(n * 100 + c * 10 + w)
    f0 = (torch.rand(n, 2, h, w, generator=g) - 0.5) * 3.0
    f0[0] += torch.tensor([0.6, -0.8]).view(2, 1, 1)                   # taps beyond the border
    f0[-1, :, 0, 0] = 0.0                                              # an exactly-zero vector ('s': occlusion rule)
    m = torch.rand(n, h, w, generator=g) > 0.2
    assert _native.splat_sum(f0.to(dev), torch.rand(n, c, h, w).to(dev)) is None
    if op.startswith('apply'):
        ref = op[-1]
        img0 = torch.rand(1 if bcast else n, c, h, w, generator=g)
        wts = torch.randn(n, c, h, w, generator=g)
        fa, ia = f0.to(dev).requires_grad_(), img0.to(dev).requires_grad_()
        (ofl.Flow(fa, ref, m.to(dev)).apply(ia) * wts.to(dev)).sum().backward()
        if ref == 't':
            assert "warp_grad_kernel" in _kernel(), _kernel()
        fb, ib = f0.clone().requires_grad_(), img0.clone().requires_grad_()
        (RFlow(fb, ref, m).apply(ib) * wts).sum().backward()
        _close(ia.grad, ib.grad, "%s W=%d: grad wrt target" % (op, w))
        _close(fa.grad, fb.grad, "%s W=%d: grad wrt flow" % (op, w), rtol=POS_RTOL)
        return
    ref = op[-1]
    f1 = (torch.rand(1 if bcast else n, 2, h, w, generator=g) - 0.5) * 2.0
    if bcast:                                                          # mode 3 needs equal shapes: a batch-1 field repeated
        f1 = f1.expand(n, -1, -1, -1)
    wts = torch.randn(n, 2, h, w, generator=g)
    fa, fb = f0.to(dev).requires_grad_(), f1.contiguous().to(dev).requires_grad_()
    out = ofl.Flow(fa, ref, m.to(dev)).combine_with(ofl.Flow(fb, ref), 3)
    (out.vecs * wts.to(dev)).sum().backward()
    if ref == 's':
        # self + self.invert('t').apply(other): the gradient wrt `other` is the warp's gradient wrt its image
        assert "warp_grad_kernel" in _kernel(), _kernel()
    ca, cb = f0.clone().requires_grad_(), f1.contiguous().clone().requires_grad_()
    exp = RFlow(ca, ref, m).combine_with(RFlow(cb, ref), 3)
    assert torch.equal(out.mask.cpu(), exp.mask)
    (exp.vecs * wts).sum().backward()
    _close(fa.grad, ca.grad, "%s W=%d: grad wrt self" % (op, w), rtol=POS_RTOL)
    _close(fb.grad, cb.grad, "%s W=%d: grad wrt other" % (op, w), rtol=POS_RTOL)


def test_narrow_frame_warp_gradient_wrt_source_direct(dev):
    """ofl_warp_bwd_grad_f32 with the gradient wrt the source on a W = 3 frame, a broadcast source and both flow signs: the
    atomics kernel against grad_ref's grid_sample autograd, tap by tap."""
    from oflibpytorch_amd import _native
    n, c, h, w = 3, 3, 9, 3
    g = torch.Generator().manual_seed(77)
    f = (torch.rand(n, 2, h, w, generator=g) - 0.5) * 4.0
    src = torch.rand(1, c, h, w, generator=g)
    gout = torch.randn(n, c, h, w, generator=g)
    for sign in (1.0, -1.0):
        gs, gf = _native.warp_bwd_grad(f.to(dev), src.to(dev), gout.to(dev), flow_sign=sign, want_src=True, want_flow=True)
        assert "warp_grad_kernel" in _kernel(), _kernel()
        fb, sb = (f * sign).clone().requires_grad_(), src.clone().requires_grad_()
        (grad_ref._ref_apply_t(fb, sb) * gout).sum().backward()
        _close(gs, sb.grad, "grad wrt source, sign %+d" % sign)
        _close(gf * sign, fb.grad, "grad wrt flow, sign %+d" % sign, rtol=POS_RTOL)


# ------------------------------------------------------------------------------------------------
# c. track_pts / Flow.track
# ------------------------------------------------------------------------------------------------
def _points(n, h, w, m, seed):
    """M points (y, x): uniform, exact integers, on row h - 1 and column w - 1, within half a pixel outside, far outside."""
    g = torch.Generator().manual_seed(seed)
    k = m // 8
    size = torch.tensor([h - 1.0, w - 1.0])
    parts = [torch.rand(n, m - 7 * k, 2, generator=g) * size,
             torch.floor(torch.rand(n, k, 2, generator=g) * size),                       # exact integers
             torch.stack([torch.full((n, k), h - 1.0), torch.rand(n, k, generator=g) * (w - 1)], -1),   # last row
             torch.stack([torch.rand(n, k, generator=g) * (h - 1), torch.full((n, k), w - 1.0)], -1),   # last column
             torch.stack([torch.full((n, k), h - 1.0), torch.floor(torch.rand(n, k, generator=g) * w)], -1),
             -torch.rand(n, k, 2, generator=g) * 0.5,                                    # half a pixel before the frame
             size + torch.rand(n, k, 2, generator=g) * 0.5,                              # half a pixel beyond it
             (torch.rand(n, k, 2, generator=g) - 0.5) * 4 * size]                        # far outside (and inside)
    pts = torch.cat(parts, 1)
    return pts[:, torch.randperm(pts.shape[1], generator=g)].contiguous()


@pytest.mark.parametrize("ref", ['s', 't'])
def test_track_pts_forward_bit_exact_against_the_oracle(ref, dev):
    """sample_pts_kernel<false> (and for 't' the splat of the flow to its start points): float points of every edge kind,
    N-M-2, M-2 and 1-M-2 broadcast forms, integer points with and without int_out -- bit for bit against oracle.track_pts."""
    import oflibpytorch_amd as ofl
    from oracle import oracle
    n, h, w, m = 4, 270, 480, 50000
    f = _field(n, h, w, 4.0, 51)
    pts = _points(n, h, w, m, 52)
    fd = f.to(dev)
    got = ofl.track_pts(fd, ref, pts.to(dev))
    assert "sample_pts_kernel<false>" in _kernel(), _kernel()
    assert np.array_equal(got.cpu().numpy(), oracle.track_pts(f.numpy(), ref, pts.numpy()))
    got2 = ofl.track_pts(fd, ref, pts[0].to(dev))                                     # M-2: every flow, the same points
    assert np.array_equal(got2.cpu().numpy(), oracle.track_pts(f.numpy(), ref, pts[:1].numpy()))
    got1 = ofl.track_pts(fd, ref, pts[1:2].to(dev))                                   # 1-M-2
    assert np.array_equal(got1.cpu().numpy(), oracle.track_pts(f.numpy(), ref, pts[1:2].numpy()))
    got0 = ofl.Flow(fd[:1], ref).track(pts[0].to(dev))                                # Flow.track, M-2 on one flow
    assert np.array_equal(got0.cpu().numpy(), oracle.track_pts(f[:1].numpy(), ref, pts[:1].numpy())[0])
    ip = torch.stack([torch.randint(0, h, (n, m)), torch.randint(0, w, (n, m))], -1)
    ip[:, :4] = torch.tensor([[0, 0], [h - 1, w - 1], [h - 1, 0], [0, w - 1]])
    for int_out in (False, True):
        gi = ofl.track_pts(fd, ref, ip.to(dev), int_out)
        ei = oracle.track_pts(f.numpy(), ref, ip.numpy(), int_out)
        assert gi.dtype == (torch.int64 if int_out else torch.float32)
        assert np.array_equal(gi.cpu().numpy(), ei)


@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("form", ['nm2', 'm2', 'bcast'])
def test_track_pts_gradients(ref, form, dev):
    """sample_pts_kernel<true>: the flow gradient scattered with atomics (4 taps x 2 planes per point), the point gradient
    through normalise_coords; for 't' also the splat backward of the field.  Broadcast points (M-2 and 1-M-2) sum their
    gradient over the batch."""
    import oflibpytorch_amd as ofl
    n, h, w, m = 4, 270, 480, 50000
    f0 = _field(n, h, w, 4.0, 61)
    p_all = _points(n, h, w, m, 62)
    p0 = {'nm2': p_all, 'm2': p_all[0], 'bcast': p_all[:1]}[form].contiguous()
    wts = torch.randn(n, m, 2, generator=torch.Generator().manual_seed(63))
    fa, pa = f0.to(dev).requires_grad_(), p0.to(dev).requires_grad_()
    out = ofl.track_pts(fa, ref, pa)
    (out * wts.to(dev)).sum().backward()
    if ref == 's':
        assert "sample_pts_kernel<true>" in _kernel(), _kernel()
    fb, pb = f0.clone().requires_grad_(), p0.clone().requires_grad_()
    (grad_ref.track_pts(fb, ref, pb) * wts).sum().backward()
    assert pa.grad.shape == p0.shape
    _close(fa.grad, fb.grad, "track %s %s: grad wrt flow" % (ref, form))
    _close(pa.grad, pb.grad, "track %s %s: grad wrt points" % (ref, form), rtol=POS_RTOL)


@pytest.mark.parametrize("ref", ['s', 't'])
def test_track_pts_crowded_cell(ref, dev):
    """20 000 points in one 2 x 2 cell: the flow gradient of its four pixels is a 20 000-term atomic sum per plane."""
    import oflibpytorch_amd as ofl
    n, h, w, m = 2, 64, 96, 20000
    f0 = _field(n, h, w, 3.0, 71, shift=False)
    g = torch.Generator().manual_seed(72)
    p0 = torch.tensor([30.0, 41.0]) + torch.rand(n, m, 2, generator=g) * 0.999
    wts = torch.rand(n, m, 2, generator=g) + 0.5                       # one sign: the sum is not a cancellation
    fa, pa = f0.to(dev).requires_grad_(), p0.to(dev).requires_grad_()
    (ofl.Flow(fa, ref).track(pa) * wts.to(dev)).sum().backward()
    fb, pb = f0.clone().requires_grad_(), p0.clone().requires_grad_()
    (RFlow(fb, ref).track(pb) * wts).sum().backward()
    if ref == 's':
        assert int((fb.grad != 0).sum()) == n * 2 * 4                 # all of it lands on the four pixels of the cell
    _close(fa.grad, fb.grad, "crowded %s: grad wrt flow" % ref)
    _close(pa.grad, pb.grad, "crowded %s: grad wrt points" % ref, rtol=POS_RTOL)


# ------------------------------------------------------------------------------------------------
# d. get_padding: flow_extents_kernel
# ------------------------------------------------------------------------------------------------
def _pad_flow(n, h, w, seed):
    """A smooth flow with the threshold's edge cases written into it: exactly +-1e-3, the float just below 1e-3, -0.0, and a
    large negative position."""
    f = _smooth(n, h, w, 3.0, seed)
    thr = np.float32(1e-3)
    below = np.nextafter(thr, np.float32(0))
    vals = torch.tensor([thr, -thr, below, -below, -0.0, 0.0], dtype=torch.float32)
    g = torch.Generator().manual_seed(seed + 1)
    k = torch.randint(0, h * w, (n, 2, max(h * w // 4, 1)), generator=g)
    flat = f.view(n, 2, -1)
    flat.scatter_(2, k, vals[torch.randint(0, len(vals), k.shape, generator=g)])
    f[:, :, 0, 0] = torch.tensor([thr, -thr]).view(1, 2)               # the first pixel: exactly on the threshold
    if h * w > 4:
        f[:, :, 0, 1] = torch.tensor([below, -below]).view(1, 2)
        f[:, :, 1 % h, 0] = -0.0
    return f.contiguous()


def _masks(kind, n, h, w, seed):
    if kind == 'full':
        return torch.ones(n, h, w, dtype=torch.bool)
    if kind == 'holes':
        return _holes(n, h, w, seed)
    m = torch.zeros(n, h, w, dtype=torch.bool)
    if kind == 'first':
        m[:, 0, 0] = True
    else:                                                              # 'last' and 'last_extreme'
        m[:, h - 1, w - 1] = True
        m[:, :h // 2, :w // 2] |= kind == 'last_extreme'
    return m


def _check_padding(f, m, ref, dev):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _native
    from oracle import oracle
    n = f.shape[0]
    sign = 1.0 if ref == 't' else -1.0
    got = _native.flow_extents(f.to(dev), m.to(dev), sign).cpu().numpy()
    assert "flow_extents_kernel" in _kernel(), _kernel()
    exp = oracle.flow_extents(f.numpy(), m.numpy(), sign)
    # bit for bit, except that -0.0 and +0.0 count as equal: a position -(0 - 0) is -0.0, the kernel's order-preserving integers
    # put -0.0 below +0.0 while NumPy's min may return either zero -- ceil(max(-lo, 0)) cannot tell them apart
    same = (got == exp) & ((np.signbit(got) == np.signbit(exp)) | (got == 0))
    assert same.all(), (got[~same.all(1)], exp[~same.all(1)])
    fl = ofl.Flow(f.to(dev), ref, m.to(dev))
    rf = RFlow(f, ref, m)
    assert fl.get_padding() == rf.get_padding()
    for k in sorted({0, n - 1}):
        assert fl.get_padding(item=k) == rf.get_padding(item=k)


@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("shape", [(3, 37, 131), (2, 5, 4), (1, 2, 2)])
@pytest.mark.parametrize("kind", ['full', 'holes', 'first', 'last', 'last_extreme'])
def test_get_padding_edges(kind, shape, ref, dev):
    """flow_extents_kernel on odd frames: the threshold's boundary (strict < at exactly 1e-3), -0.0, one valid pixel at
    (0, 0) or (h - 1, w - 1), and the extreme position on the last pixel."""
    n, h, w = shape
    f = _pad_flow(n, h, w, 81 + h)
    if kind == 'last_extreme':
        f[:, :, h - 1, w - 1] = torch.tensor([-40.0, -30.0]).view(1, 2) * (1.0 if ref == 't' else -1.0)
    _check_padding(f, _masks(kind, n, h, w, 82), ref, dev)


@pytest.mark.parametrize("ref", ['s', 't'])
def test_get_padding_1080p_batch(ref, dev):
    """B = 8 1080p: the grid-stride loop (1024 blocks per image for 2 million pixels), several images in one launch, one image
    per mask kind, large negative positions, and the extreme of image 0 on the very last pixel the loop visits."""
    n, h, w = 8, 1080, 1920
    f = _pad_flow(n, h, w, 91)
    f[2] -= 400.0                                                      # large negative positions
    s = 1.0 if ref == 't' else -1.0
    f[0, :, h - 1, w - 1] = torch.tensor([-250.0, -90.0]) * s
    m = torch.stack([_masks(k, 1, h, w, 92 + i)[0] for i, k in
                     enumerate(['full', 'holes', 'full', 'first', 'last', 'last_extreme', 'holes', 'full'])])
    _check_padding(f, m, ref, dev)


def test_get_padding_all_false_raises(dev):
    import oflibpytorch_amd as ofl
    m = torch.ones(2, 12, 16, dtype=torch.bool)
    m[1] = False
    fl = ofl.Flow(_smooth(2, 12, 16, 2.0, 3).to(dev), 't', m.to(dev))
    with pytest.raises(RuntimeError):
        fl.get_padding()
    assert fl.get_padding(item=0) == RFlow(fl.vecs.cpu(), 't', m).get_padding(item=0)
