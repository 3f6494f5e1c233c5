"""GPU tier: Flow.apply / apply_flow 't' of a feature tensor stored channels_last (N-H-W-C) runs on the N-H-W-C kernel
(ofl_warp_bwd_nhwc) and equals the planar route BIT FOR BIT.

The yardstick everywhere is the planar route on the same device: the same call on `target.contiguous()`, which the existing tests pin
to the oracle.  Values are compared on their raw bit patterns (where the target holds NaN: NaN positions, and every other bit), valid
areas as bool.  After every native case the library must name the new kernel on the target's storage type, and the result must be
channels_last-contiguous with the target's dtype.  Flows are built as in test_gpu_half_warp.py (smooth, an exactly-zero disc, corner
blocks of +-30 that leave the frame; amplitude and blocks scaled down on frames of a few pixels so that taps stay inside), plus an
integer-valued flow (weights exactly 0 and 1) and one that lands exactly on the last row and column (far taps outside, weight 0)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
STORAGE = {torch.float32: "<float,", torch.float16: "half_t", torch.bfloat16: "bf16_t"}
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
KERNEL = "warp_bwd_nhwc_kernel"


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


def _native_ran(got, target):
    name = _last()
    assert KERNEL in name and STORAGE[target.dtype] in name, "not the N-H-W-C kernel on %s: %s" % (target.dtype, name)
    assert got.dtype == target.dtype and got.is_contiguous(memory_format=CL), (got.dtype, got.stride())


def _same_bits(got, ref, what=""):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    a, b = got.contiguous().view(BITS[got.dtype]), ref.contiguous().view(BITS[ref.dtype])
    nan = torch.isnan(ref.contiguous())
    assert torch.equal(torch.isnan(got.contiguous()), nan), what
    assert torch.equal(a[~nan], b[~nan]), what


def _apply_both(vecs, target, *, flow_mask=None, target_mask=None, valid=False):
    """Flow.apply on the channels_last target (native) against the planar route on target.contiguous()."""
    import oflibpytorch_amd as ofl
    f = ofl.Flow(vecs, 't', flow_mask)
    kw = dict(target_mask=target_mask, return_valid_area=valid) if valid else {}
    got = f.apply(target, **kw)
    _native_ran(got[0] if valid else got, target)
    planar = target.contiguous()
    assert planar.is_contiguous()
    ref = f.apply(planar, **kw)
    assert KERNEL not in _last()
    if valid:
        assert got[1].dtype == torch.bool and got[1].shape == ref[1].shape and torch.equal(got[1], ref[1])
        got, ref = got[0], ref[0]
    _same_bits(got, ref)


# ---- (1) bit-exact values ----------------------------------------------------------------------------------------------
# C = 4: one lane per pixel; 12: three lanes per pixel (pixels straddle waves); 64: 16 lanes fp32, 8 lanes of 8 elements 16-bit;
# 260: 65 lanes per pixel -- a pixel spans more than one wave.  Every C at (5, 7) and (37, 53), every frame at C = 12.
CASES = [(c, hw) for c in (4, 12, 64, 260) for hw in ((5, 7), (37, 53))] + [(12, (2, 2)), (12, (96, 136))]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("c,frame", CASES, ids=str)
def test_channels_last_targets_equal_the_planar_route_bit_for_bit(c, frame, dtype, dev):
    h, w = frame
    t = _target(3, c, h, w, dtype, dev)
    for kind in ("smooth", "integer", "edge"):
        vecs = _flow(3, h, w, dev, kind)
        _apply_both(vecs, t)                               # N = 3
        _apply_both(vecs[:1], t[:1])                       # N = 1
        _apply_both(vecs, t, valid=True)


# ---- (2) masks, broadcast ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_masks_with_holes_give_the_same_values_and_valid_area(dtype, dev):
    n, c, h, w = 3, 12, 37, 53
    t, tm, fm = _target(n, c, h, w, dtype, dev, seed=1), _holes(n, h, w, dev, 1), _holes(n, h, w, dev, 2)
    for kind in ("smooth", "edge"):
        vecs = _flow(n, h, w, dev, kind)
        _apply_both(vecs, t, target_mask=tm, valid=True)
        _apply_both(vecs, t, flow_mask=fm, valid=True)
        _apply_both(vecs, t, flow_mask=fm, target_mask=tm, valid=True)
    _apply_both(_flow(n, h, w, dev), t, flow_mask=fm)      # (the flow mask without the valid area: not read)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_batch_1_target_broadcasts_under_3_flows(dtype, dev):
    n, c, h, w = 3, 12, 37, 53
    t = _target(1, c, h, w, dtype, dev, seed=2)
    vecs = _flow(n, h, w, dev)
    _apply_both(vecs, t)
    _apply_both(vecs, t, valid=True)
    _apply_both(vecs, t, target_mask=_holes(1, h, w, dev, 3), flow_mask=_holes(n, h, w, dev, 4), valid=True)
    _apply_both(vecs[:1], _target(n, c, h, w, dtype, dev, seed=2))          # and one flow under 3 targets


# ---- (3) non-finite targets --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_nan_and_infinities_come_out_as_on_the_planar_route(dtype, dev):
    import oflibpytorch_amd as ofl
    n, c, h, w = 2, 12, 40, 52
    t = _target(n, c, h, w, dtype, dev, seed=5)
    t[0, 0, 5:9, 7:11] = float('nan')
    t[0, 1, 20, 30] = float('inf')
    t[1, 2, 11, 12:20] = float('-inf')
    t[1, 0, 30, 40] = float('inf')
    t[1, 0, 30, 41] = float('-inf')                       # (inf next to -inf: a NaN where both are blended)
    t[0, 11, 3, 3] = torch.finfo(dtype).max
    t[1, 5, 25, 8] = float('inf')                         # (met by the integer flow with weights 0 and 1: inf * 0 beside it)
    assert t.is_contiguous(memory_format=CL)
    for kind in ("smooth", "integer"):
        vecs = _flow(n, h, w, dev, kind)
        got = ofl.Flow(vecs, 't').apply(t)
        _native_ran(got, t)
        ref = ofl.Flow(vecs, 't').apply(t.contiguous())
        assert KERNEL not in _last()
        assert torch.isnan(ref).any() and torch.isinf(ref).any()
        _same_bits(got, ref)


# ---- (4) apply_flow ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_apply_flow_t_takes_the_same_route(dtype, dev):
    import oflibpytorch_amd as ofl
    n, c, h, w = 3, 12, 37, 53
    vecs, t = _flow(n, h, w, dev), _target(n, c, h, w, dtype, dev, seed=3)
    got = ofl.apply_flow(vecs, t, 't')
    _native_ran(got, t)
    ref = ofl.apply_flow(vecs, t.contiguous(), 't')
    assert KERNEL not in _last()
    _same_bits(got, ref)
    got = ofl.apply_flow(vecs[:1], t, 't')                 # one flow under 3 targets
    _native_ran(got, t)
    _same_bits(got, ofl.apply_flow(vecs[:1], t.contiguous(), 't'))


# ---- (5) declined inputs keep today's route and result -----------------------------------------------------------------
def test_declined_inputs_keep_the_planar_route(dev):
    import oflibpytorch_amd as ofl
    n, h, w = 2, 37, 53
    vecs = _flow(n, h, w, dev)
    f = ofl.Flow(vecs, 't')

    def planar(got, ref):
        assert KERNEL not in _last()
        assert got.dtype == ref.dtype and got.shape == ref.shape and got.is_contiguous()
        assert torch.equal(got, ref)

    t6 = _target(n, 6, h, w, torch.float32, dev)                                       # C = 6
    got = f.apply(t6)
    name = _last()
    planar(got, f.apply(t6.contiguous()))
    assert KERNEL not in name
    t8 = _target(n, 8, h, w, torch.float32, dev)
    u8 = (t8 * 20 + 128).clamp(0, 255).to(torch.uint8).contiguous(memory_format=CL)    # uint8
    got = f.apply(u8)
    name = _last()
    planar(got, f.apply(u8.contiguous()))
    assert KERNEL not in name
    pad = [2, 3, 4, 1]                                                                 # padding=
    tp = _target(n, 8, h + 5, w + 5, torch.float32, dev, seed=7)
    got = f.apply(tp, padding=pad, cut=False)
    name = _last()
    planar(got, f.apply(tp.contiguous(), padding=pad, cut=False))
    assert KERNEL not in name
    got = ofl.apply_flow(vecs, t8, 's')                                                # an 's' flow: the splat
    name = _last()
    planar(got, ofl.apply_flow(vecs, t8.contiguous(), 's'))
    assert KERNEL not in name
    sl = _target(n, 12, h, w, torch.float32, dev)[:, 4:]                               # a channel-sliced view of a channels_last tensor
    assert sl.shape[1] == 8 and not sl.is_contiguous(memory_format=CL)
    got = f.apply(sl)
    name = _last()
    planar(got, f.apply(sl.contiguous()))
    assert KERNEL not in name
    nchw = t8.contiguous()                                                             # N-C-H-W contiguous
    got = f.apply(nchw)
    assert KERNEL not in _last() and got.is_contiguous()
    _same_bits(f.apply(t8), got)                                                       # (and the native route agrees with it)


# ---- (6) element offsets past 2^31 -------------------------------------------------------------------------------------
def test_element_offsets_past_2_to_the_31(dev):
    """fp16, N = 2, C = 64, 4096 x 4100: N * C * H * W = 2 149 580 800 > 2^31.  The last image of the batch against a launch on that image
    alone (whose offsets stay below 2^30)."""
    import oflibpytorch_amd as ofl
    n, c, h, w = 2, 64, 4096, 4100
    assert n * c * h * w > 2 ** 31
    vecs = _flow(n, h, w, dev)
    t = torch.empty((n, c, h, w), dtype=torch.float16, device=dev, memory_format=CL)
    t.view(torch.int16).random_(-15000, 15000)             # (finite fp16 bit patterns: exponent field below 31)
    got = ofl.apply_flow(vecs, t, 't')
    _native_ran(got, t)
    last = t[1:]
    assert last.is_contiguous(memory_format=CL) and not last.is_contiguous()
    alone = ofl.apply_flow(vecs[1:], last, 't')
    _native_ran(alone, t)
    assert torch.equal(got[1:].view(torch.int16), alone.view(torch.int16))
    del got, alone
    _FLOWS.pop((n, h, w))


# ---- (7) autograd ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_autograd_runs_the_native_forward_and_gives_the_planar_routes_gradients(dtype, dev):
    import oflibpytorch_amd as ofl
    n, c, h, w = 3, 8, 20, 28
    vecs, t = _flow(n, h, w, dev), _target(n, c, h, w, dtype, dev, seed=9)
    plain = ofl.apply_flow(vecs, t, 't')
    v1, t1 = vecs.clone().requires_grad_(True), t.clone().requires_grad_(True)
    assert t1.is_contiguous(memory_format=CL) and not t1.is_contiguous()
    out = ofl.apply_flow(v1, t1, 't')
    _native_ran(out, t)
    assert out.requires_grad
    _same_bits(out.detach(), plain)
    g = torch.randn(out.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(3)).to(dtype)
    out.backward(g)
    v2, t2 = vecs.clone().requires_grad_(True), t.contiguous().clone().requires_grad_(True)
    assert t2.is_contiguous()
    out2 = ofl.apply_flow(v2, t2, 't')
    assert KERNEL not in _last()
    _same_bits(out.detach(), out2.detach())
    out2.backward(g)
    assert t1.grad.dtype == dtype and v1.grad.dtype == torch.float32
    assert t1.grad.is_contiguous(memory_format=CL) and not t1.grad.is_contiguous(), "the source gradient is not channels_last"
    _same_bits(t1.grad, t2.grad, "gradient wrt the target")
    assert torch.equal(v1.grad.view(torch.int32), v2.grad.view(torch.int32)), "gradient wrt the flow"
    # through Flow.apply too, only the target requiring a gradient
    t3 = t.clone().requires_grad_(True)
    out3 = ofl.Flow(vecs, 't').apply(t3)
    _native_ran(out3, t)
    out3.backward(g)
    assert t3.grad.is_contiguous(memory_format=CL)
    _same_bits(t3.grad, t2.grad, "gradient wrt the target (Flow.apply)")
