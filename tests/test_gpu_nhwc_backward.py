"""GPU tier: the backward of Flow.apply / apply_flow 't' on a channels_last feature tensor with a channels_last upstream gradient
(DESIGN.md 3.14 "Autograd") -- the flow gradient from the N-H-W-C storage (ofl_warp_bwd_grad_nhwc), the target gradient through the
library's own layout copies (ofl_nhwc_to_planes, ofl_planes_to_nhwc) around the planar gather splat -- equals the planar route BIT FOR
BIT and allocates no transposed copy of the source.

The yardstick is the planar route on the same device: the same call on `.contiguous()` copies, which the existing tests pin to the
oracle and to tests/grad_ref.py; one case goes against grad_ref directly.  Flows and targets are built as in test_gpu_nhwc_warp.py."""

import pytest
import torch

import case_runner
import grad_ref

pytestmark = pytest.mark.gpu

CL = torch.channels_last
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
STORAGE = {torch.float32: "<float,", torch.float16: "half_t", torch.bfloat16: "bf16_t"}
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
ELEM = {4: "unsigned int", 2: "unsigned short"}
K_FLOW, K_COPY, K_FWD = "warp_grad_flow_nhwc_kernel", "nhwc_transpose_kernel", "warp_bwd_nhwc_kernel"
CHANNELS = (4, 12, 64, 260)          # one chunk; three; a whole transpose tile (4-byte) and more; 260: 8 full tiles and one of 4 channels
FRAMES = ((5, 7), (37, 53), (2, 2), (96, 136))     # odd H*W below one pixel tile; several tiles with a tail; the smallest; whole tiles


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tier needs a HIP device"
    from oflibpytorch_amd import _native
    _native.load_library()
    return torch.device('cuda', 0)


_FLOWS = {}


def _flow(n, h, w, dev, kind="smooth"):
    """smooth: sigma ~ 4 random flow with an exactly-zero disc and two corner blocks whose displacements leave the frame; integer: the
    same rounded to whole pixels; edge: the same with the upper half landing exactly on the last row and the left half of the lower
    half exactly on the last column (cached)."""
    if (n, h, w) not in _FLOWS:
        g = torch.Generator().manual_seed(1000 * n + h + w)
        amp = min(4.0, min(h, w) / 3.0)
        lo = (torch.randn(n, 2, max(h // 12, 2), max(w // 12, 2), generator=g) * amp).to(dev)
        f = torch.nn.functional.interpolate(lo, size=(h, w), mode='bicubic', align_corners=True).contiguous()
        yy, xx = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing='ij')
        f[:, :, (yy - h // 2) ** 2 + (xx - w // 3) ** 2 < (min(h, w) // 6) ** 2] = 0.0
        k = min(6, h // 4, w // 4)
        if k:
            f[:, :, :k, :k] = 30.0
            f[:, :, -k:, -k:] = -30.0
        edge = f.clone()
        edge[:, 1, : h // 2] = (yy[: h // 2] - (h - 1)).float()
        edge[:, 0, h // 2:, : w // 2] = (xx[h // 2:, : w // 2] - (w - 1)).float()
        _FLOWS[(n, h, w)] = {"smooth": f, "integer": torch.round(f), "edge": edge}
    return _FLOWS[(n, h, w)][kind]


def _target(n, c, h, w, dtype, dev, seed=0):
    """random values, stored channels_last"""
    g = torch.Generator(device=dev).manual_seed(7 + seed)
    t = (torch.randn(n, c, h, w, generator=g, device=dev) * 3).to(dtype).contiguous(memory_format=CL)
    assert t.is_contiguous(memory_format=CL) and (not t.is_contiguous() or c == 1 or h * w == 1)
    return t


def _holes(n, h, w, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.rand(n, h, w, generator=g, device=dev) > 0.2


def _last():
    from oflibpytorch_amd import _native
    return _native.last_kernel_name()


def _bits(t):
    """the raw bit patterns of a tensor in logical (N, C, H, W) order"""
    return t.contiguous().view(BITS.get(t.dtype, t.dtype))


def _same_bits(got, ref, what=""):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    nan = torch.isnan(ref.contiguous())
    assert torch.equal(torch.isnan(got.contiguous()), nan), what
    assert torch.equal(_bits(got)[~nan], _bits(ref)[~nan]), what


# ---- (1) the layout copies ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=str)
@pytest.mark.parametrize("c", CHANNELS)
def test_the_layout_copies_move_every_bit_pattern(c, dtype, dev):
    from oflibpytorch_amd import _native
    size = torch.zeros((), dtype=dtype).element_size()
    for h, w in FRAMES:
        raw = torch.empty((3, c, h, w), dtype=BITS[dtype], device=dev).random_()          # every pattern: NaN payloads, infinities, denormals
        raw[0, 0, 0, 0], raw[2, c - 1, h - 1, w - 1] = 0x7FC1, -2                          # (a NaN with a payload in either width)
        planar = raw.view(dtype)
        assert torch.isnan(planar).any()
        t = planar.contiguous(memory_format=CL)
        assert t.is_contiguous(memory_format=CL) and not t.is_contiguous()
        p = _native.nhwc_to_planes(t)
        name = _last()
        assert K_COPY in name and ELEM[size] in name and ", true>" in name, name
        assert p.dtype == dtype and p.is_contiguous() and torch.equal(p.view(BITS[dtype]), raw), (c, h, w)
        q = _native.planes_to_nhwc(planar)
        name = _last()
        assert K_COPY in name and ELEM[size] in name and ", false>" in name, name
        assert q.dtype == dtype and q.is_contiguous(memory_format=CL) and not q.is_contiguous()
        assert torch.equal(_bits(q), raw) and torch.equal(q.permute(0, 2, 3, 1).contiguous().view(BITS[dtype]),
                                                          t.permute(0, 2, 3, 1).contiguous().view(BITS[dtype])), (c, h, w)
        back = _native.planes_to_nhwc(_native.nhwc_to_planes(q))                           # the round trip is the identity
        assert torch.equal(_bits(back), raw)


# ---- (2) the flow gradient, bit for bit --------------------------------------------------------------------------------
def _planar_flow_grad(vecs, s, g, **kw):
    """the planar route's flow gradient of the same values: warp_bwd_grad (fp32), warp_bwd_grad_x16 (16-bit; on a frame it declines,
    the fp32 kernels on the exactly up-converted planes, as WarpFn.backward does)"""
    from oflibpytorch_amd import _native
    sp, gp = s.contiguous(), g.contiguous()
    assert sp.is_contiguous() and gp.is_contiguous()
    res = None
    if s.dtype != torch.float32:
        res = _native.warp_bwd_grad_x16(vecs, sp, gp, want_src=False, want_flow=True, **kw)
    if res is None:
        res = _native.warp_bwd_grad(vecs, sp.float(), gp.float(), want_src=False, want_flow=True, **kw)
    assert K_FLOW not in _last()
    return res[1]


def _native_flow_grad(vecs, s, g, **kw):
    from oflibpytorch_amd import _native
    res = _native.warp_bwd_grad_nhwc(vecs, s, g, want_src=False, want_flow=True, **kw)
    assert res is not None and res[0] is None
    name = _last()
    assert K_FLOW in name and STORAGE[s.dtype] in name, name
    assert res[1].dtype == torch.float32 and res[1].is_contiguous() and res[1].shape == (s.shape[0], 2) + tuple(s.shape[2:])
    return res[1]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("c", CHANNELS)
def test_the_flow_gradient_equals_the_planar_routes_bit_for_bit(c, dtype, dev):
    n = 3
    for h, w in FRAMES:
        s, g = _target(n, c, h, w, dtype, dev, seed=1), _target(n, c, h, w, dtype, dev, seed=2)
        for kind in ("smooth", "integer", "edge"):
            vecs = _flow(n, h, w, dev, kind)
            for kw in (dict(flow_sign=1.0, g_scale=1.0), dict(flow_sign=-1.0, g_scale=1.0), dict(flow_sign=1.0, g_scale=-1.0)):
                got, ref = _native_flow_grad(vecs, s, g, **kw), _planar_flow_grad(vecs, s, g, **kw)
                assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), (c, h, w, kind, kw)
        vecs = _flow(n, h, w, dev)[:1]                                                    # one flow under 3 images
        got, ref = _native_flow_grad(vecs, s, g, flow_sign=1.0, g_scale=1.0), _planar_flow_grad(vecs, s, g, flow_sign=1.0, g_scale=1.0)
        assert got.shape[0] == n and torch.equal(got.view(torch.int32), ref.view(torch.int32)), (c, h, w, "batch-1 flow")
        bad = g.clone()                                                                   # NaN and infinities in a few pixels
        bad[0, 0, 0, 0], bad[1, c - 1, h - 1, w - 1], bad[2, 1, h // 2, w // 2] = float('nan'), float('inf'), float('-inf')
        bad[2, 2, 0, w - 1] = float('inf')
        assert bad.is_contiguous(memory_format=CL)
        vecs = _flow(n, h, w, dev)
        got, ref = _native_flow_grad(vecs, s, bad, flow_sign=1.0, g_scale=1.0), _planar_flow_grad(vecs, s, bad, flow_sign=1.0, g_scale=1.0)
        assert not torch.isfinite(ref).all()
        _same_bits(got, ref, (c, h, w, "non-finite gradient"))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_scaled_source_gradient_is_declined_before_anything_runs(dtype, dev):
    """`warp_bwd_grad_nhwc` used to hand g_scale to the gather splat as its data sign, which takes +-1 only: |g_scale| != 1 with
    want_src raised (status -3) after the first layout copy.  It is declined up front now (the planar route scales in fp32); +-1
    and the flow gradient alone are still native."""
    from oflibpytorch_amd import _native
    n, c, h, w = 2, 4, 37, 53
    vecs, s, g = _flow(n, h, w, dev), _target(n, c, h, w, dtype, dev, seed=1), _target(n, c, h, w, dtype, dev, seed=2)
    assert _native.warp_bwd_grad_nhwc(vecs, s, g, g_scale=0.5) is None
    assert _native.warp_bwd_grad_nhwc(vecs, s, g, g_scale=-2.0, want_flow=False) is None
    got = _native_flow_grad(vecs, s, g, flow_sign=1.0, g_scale=0.5)
    assert torch.equal(got.view(torch.int32), _planar_flow_grad(vecs, s, g, flow_sign=1.0, g_scale=0.5).view(torch.int32))
    gs, gf = _native.warp_bwd_grad_nhwc(vecs, s, g, g_scale=-1.0)
    rs, rf = _native.warp_bwd_grad(vecs, s.float().contiguous(), g.float().contiguous(), g_scale=-1.0)
    assert gs.is_contiguous(memory_format=CL) and gs.dtype == dtype
    assert torch.equal(gs.contiguous().view(BITS[dtype]), rs.to(dtype).view(BITS[dtype])) and torch.equal(gf, rf)


# ---- (3) the whole backward through the public API ---------------------------------------------------------------------
def _backward_both(call, vecs, t, g, *, flow_grad=True, target_grad=True):
    """`call(v, t)` on the channels_last target with the channels_last gradient against the same call on contiguous copies; returns
    the kernel named after the native backward."""
    v1 = vecs.clone().requires_grad_(flow_grad)
    t1 = t.clone(memory_format=torch.preserve_format).requires_grad_(target_grad)
    assert t1.is_contiguous(memory_format=CL) and not t1.is_contiguous() and g.is_contiguous(memory_format=CL) and not g.is_contiguous()
    out = call(v1, t1)
    assert K_FWD in _last() and out.is_contiguous(memory_format=CL)
    out.backward(g)
    name = _last()
    v2, t2 = vecs.clone().requires_grad_(flow_grad), t.contiguous().clone().requires_grad_(target_grad)
    gp = g.contiguous()
    assert t2.is_contiguous() and gp.is_contiguous()
    out2 = call(v2, t2)
    _same_bits(out.detach(), out2.detach(), "forward")
    out2.backward(gp)
    after = _last()
    assert K_FLOW not in after and K_COPY not in after, after
    if flow_grad:
        assert v1.grad.dtype == torch.float32 and torch.equal(v1.grad, v2.grad), "gradient wrt the flow"
        assert torch.equal(v1.grad.view(torch.int32), v2.grad.view(torch.int32)), "gradient wrt the flow (bits)"
    else:
        assert v1.grad is None
    if target_grad:
        assert t1.grad.dtype == t.dtype and t1.grad.is_contiguous(memory_format=CL) and not t1.grad.is_contiguous(), "not channels_last"
        _same_bits(t1.grad, t2.grad, "gradient wrt the target")
    else:
        assert t1.grad is None
    return name


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", [(3, 8, 20, 28), (3, 64, 37, 53), (2, 12, 96, 136)], ids=str)
def test_backward_through_the_public_api_equals_the_planar_routes(shape, dtype, dev):
    import oflibpytorch_amd as ofl
    n, c, h, w = shape
    vecs, t = _flow(n, h, w, dev), _target(n, c, h, w, dtype, dev, seed=9)
    g = _target(n, c, h, w, dtype, dev, seed=11)
    fm, tm = _holes(n, h, w, dev, 1), _holes(n, h, w, dev, 2)
    plain = lambda v, x: ofl.apply_flow(v, x, 't')
    masked = lambda v, x: ofl.Flow(v, 't', fm).apply(x, target_mask=tm, return_valid_area=True)[0]
    for call in (plain, masked):
        name = _backward_both(call, vecs, t, g)
        assert K_FLOW in name and STORAGE[dtype] in name, name                # (the flow gradient is launched last)
        name = _backward_both(call, vecs, t, g, target_grad=False)            # only the flow
        assert K_FLOW in name and STORAGE[dtype] in name, name
        name = _backward_both(call, vecs, t, g, flow_grad=False)              # only the target
        assert K_COPY in name and ", false>" in name, name
    name = _backward_both(plain, vecs[:1], t, g)                              # one flow under N targets: its gradient is summed
    assert K_FLOW in name


# ---- (4) against the reference's autograd ------------------------------------------------------------------------------
def test_backward_against_the_reference_op_sequence_on_the_cpu(dev):
    import oflibpytorch_amd as ofl
    n, c, h, w = 2, 8, 20, 28
    vecs, t = _flow(n, h, w, dev), _target(n, c, h, w, torch.float32, dev, seed=4)
    g = _target(n, c, h, w, torch.float32, dev, seed=5)
    v1, t1 = vecs.clone().requires_grad_(True), t.clone(memory_format=torch.preserve_format).requires_grad_(True)
    out = ofl.apply_flow(v1, t1, 't')
    out.backward(g)
    assert K_FLOW in _last()
    v0, t0 = vecs.cpu().requires_grad_(True), t.cpu().contiguous().requires_grad_(True)
    ref = grad_ref.apply_flow(v0, t0, 't')
    ref.backward(g.cpu().contiguous())
    for got, exp, what in ((v1.grad, v0.grad, "flow"), (t1.grad, t0.grad, "target")):
        scale = float(exp.abs().max())
        err = float((got.detach().cpu().double() - exp.double()).abs().max())
        print("gradient wrt the %s: max |diff| %.3g, scale %.3g" % (what, err, scale))
        assert err <= case_runner.GRAD_RTOL * max(scale, 1e-6), "%s: max |diff| %.3g against a scale of %.3g" % (what, err, scale)


# ---- (5) fallbacks keep their route and results ------------------------------------------------------------------------
def _fallback(call, vecs, t, g):
    """a case the native backward does not take: the gradients of the same call on contiguous copies, and none of the new kernels"""
    v1, t1 = vecs.clone().requires_grad_(True), t.clone(memory_format=torch.preserve_format).requires_grad_(True)
    out = call(v1, t1)
    out.backward(g)
    name = _last()
    assert K_FLOW not in name and K_COPY not in name, name
    v2, t2 = vecs.clone().requires_grad_(True), t.contiguous().clone().requires_grad_(True)
    call(v2, t2).backward(g.contiguous())
    assert torch.equal(v1.grad.view(torch.int32), v2.grad.view(torch.int32)), "gradient wrt the flow"
    assert t1.grad.shape == t.shape
    _same_bits(t1.grad, t2.grad, "gradient wrt the target")


def test_fallbacks_keep_the_planar_backward_and_its_results(dev):
    import oflibpytorch_amd as ofl
    plain = lambda v, x: ofl.apply_flow(v, x, 't')
    n, c, h, w = 3, 8, 20, 28
    vecs = _flow(n, h, w, dev)
    for dtype in (torch.float32, torch.bfloat16):
        t = _target(n, c, h, w, dtype, dev, seed=9)
        _fallback(plain, vecs, t, _target(n, c, h, w, dtype, dev, seed=3).contiguous())       # a planar upstream gradient
        _fallback(plain, vecs, t[:1], _target(n, c, h, w, dtype, dev, seed=3))                # a batch-1 target under 3 flows
        # frames the gather splat does not take (W < 4): the planar route sums the target's gradient with float atomics, whose order is
        # not fixed -- so H - 1 and W - 1 powers of two and a constant whole-pixel flow: every weight is exactly 0 or 1, every sum has at
        # most one non-zero term, and both runs give the same bits in any order
        for ww in (2, 3):
            shift = torch.zeros(n, 2, 17, ww, device=dev)
            shift[:, 0], shift[:, 1] = 1.0, -2.0
            _fallback(plain, shift, _target(n, c, 17, ww, dtype, dev), _target(n, c, 17, ww, dtype, dev, seed=3))
        _fallback(plain, vecs, _target(n, 6, h, w, dtype, dev), _target(n, 6, h, w, dtype, dev, seed=3))   # C = 6
    pad = [2, 3, 4, 1]                                                                        # padding=
    padded = lambda v, x: ofl.Flow(v, 't').apply(x, padding=pad, cut=False)
    tp = _target(n, c, h + 5, w + 5, torch.float32, dev, seed=7)
    v1, t1 = vecs.clone().requires_grad_(True), tp.clone(memory_format=torch.preserve_format).requires_grad_(True)
    out = padded(v1, t1)
    gpad = torch.randn(out.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(5)).contiguous(memory_format=CL)
    out.backward(gpad)
    name = _last()
    assert K_FLOW not in name and K_COPY not in name, name
    v2, t2 = vecs.clone().requires_grad_(True), tp.contiguous().clone().requires_grad_(True)
    padded(v2, t2).backward(gpad.contiguous())
    assert torch.equal(v1.grad, v2.grad) and torch.equal(t1.grad, t2.grad)


# ---- (6) memory --------------------------------------------------------------------------------------------------------
def _backward_peak(vecs, t, g, *, flow_grad, target_grad):
    import oflibpytorch_amd as ofl
    v1 = vecs.clone().requires_grad_(flow_grad)
    t1 = t.clone(memory_format=torch.preserve_format).requires_grad_(target_grad)
    out = ofl.apply_flow(v1, t1, 't')
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out.backward(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    assert (K_FLOW if flow_grad else K_COPY) in _last()
    return peak


def test_backward_allocates_no_transposed_copy_of_the_source(dev):
    """Bounds from sizes alone.  Only the flow: the fp32 [N, 2, H, W] result, so less than ONE feature map.  Both: the planar
    gradient, the planar result and the channels_last result (three maps; the first is released before the third is allocated) plus
    the gather splat's workspace."""
    from oflibpytorch_amd import _native
    n, c, h, w = 2, 64, 96, 136
    one_map = n * c * h * w * 4
    vecs, t, g = _flow(n, h, w, dev), _target(n, c, h, w, torch.float32, dev), _target(n, c, h, w, torch.float32, dev, seed=3)
    peak = _backward_peak(vecs, t, g, flow_grad=True, target_grad=False)
    print("only the flow: peak %d bytes above the start, one map %d" % (peak, one_map))
    assert peak < one_map
    ws = 4 * int(_native.load_library().ofl_splat_tiled_workspace_ints(n, h, w))
    peak = _backward_peak(vecs, t, g, flow_grad=True, target_grad=True)
    print("both: peak %d bytes above the start, three maps + workspace %d" % (peak, 3 * one_map + ws))
    assert peak < 3 * one_map + ws


# ---- (7) element offsets past 2^31 -------------------------------------------------------------------------------------
def test_element_offsets_past_2_to_the_31(dev):
    """bf16, N = 2, C = 128, 2900 x 2901: N * C * H * W = 2 153 702 400 > 2^31.  The layout copies and the flow-gradient primitive on
    the whole batch; the last image against the same image computed alone (whose offsets stay below 2^31)."""
    from oflibpytorch_amd import _native
    n, c, h, w = 2, 128, 2900, 2901
    assert n * c * h * w > 2 ** 31 and c * h * w < 2 ** 31
    t = torch.empty((n, c, h, w), dtype=torch.bfloat16, device=dev, memory_format=CL)
    flat = t.view(torch.int16).permute(0, 2, 3, 1).reshape(-1)     # (the storage, in its own order)
    assert flat.data_ptr() == t.data_ptr()
    flat.random_(0, 16000)                                 # finite bf16 bit patterns: exponent field below 255 ...
    flat[::3] += -32768                                    # ... every third one negative
    assert torch.isfinite(t[1, :, 5, 7]).all() and (t[1, :, 5, 7] < 0).any()
    last = t[1:]
    assert last.is_contiguous(memory_format=CL) and not last.is_contiguous()
    p = _native.nhwc_to_planes(t)
    assert K_COPY in _last() and p.is_contiguous()
    alone = _native.nhwc_to_planes(last)
    assert torch.equal(p[1:].view(torch.int16), alone.view(torch.int16))
    assert torch.equal(alone[0, :, 17, 33].view(torch.int16), last[0, :, 17, 33].view(torch.int16))
    del alone
    q = _native.planes_to_nhwc(p)
    assert K_COPY in _last() and q.is_contiguous(memory_format=CL)
    assert torch.equal(q[1:].permute(0, 2, 3, 1).view(torch.int16), last.permute(0, 2, 3, 1).view(torch.int16))
    del p
    vecs = _flow(n, h, w, dev)
    gf = _native_flow_grad(vecs, t, q, flow_sign=1.0, g_scale=1.0)
    gl = _native_flow_grad(vecs[1:], last, q[1:], flow_sign=1.0, g_scale=1.0)
    assert torch.isfinite(gf).all() and gf[1].abs().max() > 0
    assert torch.equal(gf[1:].view(torch.int32), gl.view(torch.int32))
    del gf, gl, q, t
    _FLOWS.pop((n, h, w))


# ---- (8) run to run ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_the_same_backward_twice_gives_identical_bits(dtype, dev):
    import oflibpytorch_amd as ofl
    n, c, h, w = 3, 64, 37, 53
    vecs, t, g = _flow(n, h, w, dev), _target(n, c, h, w, dtype, dev, seed=9), _target(n, c, h, w, dtype, dev, seed=11)
    grads = []
    for _ in range(2):
        v1, t1 = vecs.clone().requires_grad_(True), t.clone(memory_format=torch.preserve_format).requires_grad_(True)
        ofl.apply_flow(v1, t1, 't').backward(g)
        assert K_FLOW in _last()
        grads.append((v1.grad, t1.grad))
    assert torch.equal(grads[0][0].view(torch.int32), grads[1][0].view(torch.int32))
    assert torch.equal(_bits(grads[0][1]), _bits(grads[1][1]))
