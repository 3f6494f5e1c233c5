"""GPU tier: the backward pass of Flow.apply / apply_flow 't' on a 16-bit feature tensor runs on the native 16-bit kernels
(ofl_warp_bwd_grad_x16, ofl_splat_sum_x16: no fp32 copy of the source, of the upstream gradient or of the source gradient) and
gives the present route's gradients BIT FOR BIT.

The yardstick everywhere is that route on the same device: the same call on `target.float()`, its result `.to(dtype)`, the same
upstream gradient -- the gradient wrt the target compared on its raw 16-bit patterns, the one wrt the flow (fp32) with torch.equal.
The flows are those of test_gpu_half_warp.py (sigma ~ 4, an exactly-zero disc, two corner blocks that leave the frame): no cell of
the gather splat reaches 65 records there, so it stays on its in-order path and every result is reproducible to the bit."""
import re

import pytest
import torch

from test_gpu_half_warp import _flow, _holes, _same_bits, _target

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
TX = {torch.bfloat16: "bf16_t", torch.float16: "half_t"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tier needs a HIP device"
    from oflibpytorch_amd import _native
    _native.load_library()
    return torch.device('cuda', 0)


def _name():
    from oflibpytorch_amd import _native
    return _native.last_kernel_name()


def _is16(name):
    return "half_t" in name or "bf16_t" in name


def _is_grad16(name, dtype):
    """a GRAD instantiation of the staged kernels on TS = half_t / bf16_t (up to 3 planes), or the one-pixel-per-lane kernel (more)"""
    tx = TX[dtype]
    return bool(re.search(r"warp_bwd_rows_kernel<\d+, \d+, false, 0, false, false, %s, float, false, true>" % tx, name)
                or re.search(r"warp_bwd_lds_column_kernel<\d+, \d+, false, false, false, false, %s, float, true" % tx, name)
                or ("warp_grad_flow_x16_kernel<%s>" % tx) in name)


def _upstream(shape, dtype, dev, seed=3):
    return torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed)).to(dtype)


def _grads(vecs, t, g, *, native, flow_mask=None, target_mask=None, want=(True, True), names=None):
    """(grad wrt the target in t.dtype, grad wrt the flow in fp32) of apply_flow / Flow.apply 't' under the upstream gradient g:
    native = the call on the 16-bit target itself; else the present route, `t.float()` in and `.to(dtype)` out."""
    import oflibpytorch_amd as ofl
    v, x = vecs.clone().requires_grad_(want[1]), t.clone().requires_grad_(want[0])
    xin = x if native else x.float()
    if flow_mask is None and target_mask is None:
        out = ofl.apply_flow(v, xin, 't')
    else:
        out = ofl.Flow(v, 't', flow_mask).apply(xin, target_mask=target_mask, return_valid_area=True)[0]
    if not native:
        out = out.to(t.dtype)
    assert out.dtype == t.dtype
    out.backward(g)
    if names is not None:
        names.append(_name())
    return x.grad, v.grad


def _compare(vecs, t, g, **kw):
    names = []
    gt, gv = _grads(vecs, t, g, native=True, names=names, **kw)
    rt, rv = _grads(vecs, t, g, native=False, **kw)
    assert gt.dtype == t.dtype and gv.dtype == torch.float32
    _same_bits(gt, rt, "gradient wrt the target")
    assert torch.equal(gv, rv), "gradient wrt the flow"
    return names[0]


# ---- (1) bit-equal gradients -------------------------------------------------------------------------------------------
SHAPES = [(3, 4, 37, 53), (2, 3, 96, 136), (2, 1, 96, 136), (1, 64, 64, 96), (2, 5, 270, 480)]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gradients_equal_the_fp32_route_bit_for_bit(shape, dtype, dev):
    n, c, h, w = shape
    vecs, t, g = _flow(n, h, w, dev), _target(n, c, h, w, dtype, dev, seed=9), _upstream(shape, dtype, dev)
    assert _is16(_compare(vecs, t, g))
    # through Flow.apply with holes in both masks and the valid area
    assert _is16(_compare(vecs, t, g, flow_mask=_holes(n, h, w, dev, 2), target_mask=_holes(n, h, w, dev, 1)))


# ---- (2) the native kernels ran ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", [(2, 3, 96, 136), (2, 2, 37, 53), (2, 5, 64, 96)], ids=str)
def test_the_native_16_bit_kernels_ran(shape, dtype, dev):
    n, c, h, w = shape
    vecs, t, g = _flow(n, h, w, dev), _target(n, c, h, w, dtype, dev, seed=4), _upstream(shape, dtype, dev, seed=5)
    names = []
    _grads(vecs, t, g, native=True, want=(False, True), names=names)          # only the flow wants a gradient
    assert _is_grad16(names[0], dtype), names[0]
    _grads(vecs, t, g, native=True, want=(True, False), names=names)          # only the target does
    assert "splat_" in names[1] and ("SpMixed<%s>" % TX[dtype]) in names[1], names[1]
    _grads(vecs, t.float(), g.float(), native=True, want=(False, True), names=names)      # an fp32 source: neither
    _grads(vecs, t.float(), g.float(), native=True, want=(True, False), names=names)
    assert not _is16(names[2]) and not _is16(names[3]), names[2:]


# ---- (3) no fp32 transients --------------------------------------------------------------------------------------------
def test_backward_makes_no_fp32_copies(dev):
    """Peak memory over `backward` above the level before it, against a bound from sizes alone: the 16-bit source gradient, the
    fp32 flow gradient, the gather splat's workspace and fallback accumulator as the library sizes them, and half as much again for
    the allocator's rounding.  The copy route holds the fp32 source, the fp32 upstream gradient and the fp32 source gradient at
    once: at least 12 bytes per element."""
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _native
    lib = _native.load_library()
    n, c, h, w = 2, 32, 270, 480
    dtype = torch.bfloat16
    vecs, t, g = _flow(n, h, w, dev), _target(n, c, h, w, dtype, dev), _upstream((n, c, h, w), dtype, dev)
    ws = 4 * int(lib.ofl_splat_tiled_workspace_ints(n, h, w))
    planes = 1 + 3
    accum = 4 * int(lib.ofl_splat_tiled_fallback_images(n, planes, h, w)) * planes * h * w
    bound = 1.5 * (2 * t.numel() + 4 * vecs.numel() + ws + accum)
    assert bound < 8 * t.numel(), (bound, 8 * t.numel())

    def step(measure):
        v, x = vecs.clone().requires_grad_(True), t.clone().requires_grad_(True)
        out = ofl.apply_flow(v, x, 't')
        torch.cuda.synchronize(dev)
        if measure:
            torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        out.backward(g)
        torch.cuda.synchronize(dev)
        return torch.cuda.max_memory_allocated(dev) - before, x.grad, v.grad
    step(False)                                            # (warm: the library's own first-call allocations)
    peak, gx, gv = step(True)
    assert gx.dtype == dtype and gv.dtype == torch.float32
    print("peak over backward: %d bytes; bound %d; 8 B / element %d; the copy route needs %d" % (peak, bound, 8 * t.numel(), 12 * t.numel()))
    assert peak < bound, "peak %d bytes above the level before backward; bound %d, fp32 copies need %d" % (peak, bound, 12 * t.numel())


# ---- (4) rounding ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_source_gradient_on_and_next_to_rounding_ties(dtype, dev):
    """Whole-pixel and half-pixel flows make every bilinear weight 1, 0.5 or 0.25; an upstream gradient of integers with every
    mantissa bit of the format in use (p = 8 / 11 significant bits) then makes fp32 sums that need one / two bits more than the
    format holds: exact ties (fraction .5 of the format's ulp) and their neighbours below and above (.25, .75).  The source gradient
    is `fp32_sum.to(dtype)`: round to nearest even."""
    import oflibpytorch_amd as ofl
    n, c, h, w = 2, 3, 40, 52
    p = 8 if dtype == torch.bfloat16 else 11
    gen = torch.Generator(device=dev).manual_seed(11)
    g = torch.randint(2 ** (p - 1), 2 ** p, (n, c, h, w), generator=gen, device=dev).to(dtype)
    assert torch.equal(g.float().to(dtype), g)
    g[:, 1] = -g[:, 1]
    g[:, 2] = g[:, 2] / 64
    vecs = torch.zeros(n, 2, h, w, device=dev)
    vecs[:, 0, :, : w // 3] = 0.5                        # half a pixel in x ...
    vecs[:, 0, :, w // 3: 2 * w // 3] = 1.0              # ... a whole pixel ...
    vecs[:, 0, :, 2 * w // 3:] = -2.0
    vecs[:, 1, h // 2:] = 0.5                            # ... and half a pixel in y on top: weights 0.25
    vecs[1] = -vecs[1]
    t = _target(n, c, h, w, dtype, dev, seed=8)
    x32 = t.float().requires_grad_(True)
    ofl.apply_flow(vecs, x32, 't').backward(g.float())
    sums = x32.grad                                       # the fp32 sums themselves
    drop = 16 if dtype == torch.bfloat16 else 13          # mantissa bits of the fp32 sum the format drops (normal values on both sides)
    low = sums.view(torch.int32) & ((1 << drop) - 1)
    assert (low == 1 << (drop - 1)).any(), "no sum on a tie"
    assert (low == 1 << (drop - 2)).any() and (low == 3 << (drop - 2)).any(), "no sum just below / above a tie"
    x = t.clone().requires_grad_(True)
    ofl.apply_flow(vecs, x, 't').backward(g)
    assert "SpMixed<%s>" % TX[dtype] in _name()
    _same_bits(x.grad, sums.to(dtype), "source gradient against fp32_sum.to(dtype)")


# ---- (5) NaN and infinities --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_nan_and_infinities_come_out_as_the_fp32_route_gives_them(dtype, dev):
    n, c, h, w = 2, 3, 40, 52
    vecs, t, g = _flow(n, h, w, dev), _target(n, c, h, w, dtype, dev, seed=5), _upstream((n, c, h, w), dtype, dev, seed=6)
    for z in (t, g):
        z[0, 0, 5:9, 7:11] = float('nan')
        z[0, 1, 20, 30] = float('inf')
        z[1, 2, 11, 12:20] = float('-inf')
        z[1, 0, 30, 40] = float('inf')
        z[1, 0, 30, 41] = float('-inf')                   # (inf next to -inf: a NaN where both are blended)
        z[0, 2, 3, 3] = torch.finfo(dtype).max
    g = g.roll(9, dims=3).contiguous()                    # (the two patterns do not sit on top of each other)
    gt, gv = _grads(vecs, t, g, native=True)
    rt, rv = _grads(vecs, t, g, native=False)
    for got, ref, bits in ((gt, rt, torch.int16), (gv, rv, torch.int32)):
        nan = torch.isnan(ref)
        assert nan.any() and torch.equal(torch.isnan(got), nan)
        assert torch.equal(got.view(bits)[~nan], ref.view(bits)[~nan])
    assert torch.isinf(rt).any()


# ---- (6) declined calls ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_declined_calls_take_the_present_route(dtype, dev):
    import oflibpytorch_amd as ofl
    # a (1, C, H, W) target under a batch of 3 flows: its gradient is summed over the batch in fp32
    n, c, h, w = 3, 4, 40, 52
    vecs, t, g = _flow(n, h, w, dev), _target(1, c, h, w, dtype, dev, seed=6), _upstream((n, c, h, w), dtype, dev)
    assert not _is16(_compare(vecs, t, g))
    # frames the staged kernels do not take
    # (their source gradient is the float-atomics kernel's: half-pixel and whole-pixel shifts along x give every source pixel at most two
    # non-zero contributions, whose sum does not depend on the order they arrive in)
    for ww in (3, 2):
        vecs = torch.zeros(2, 2, 24, ww, device=dev)
        vecs[0, 0], vecs[1, 0] = 0.5, -1.0
        t, g = _target(2, 3, 24, ww, dtype, dev, seed=7), _upstream((2, 3, 24, ww), dtype, dev)
        assert not _is16(_compare(vecs, t, g))
    # a channels-last upstream gradient (made contiguous by the backward pass)
    n, c, h, w = 2, 4, 40, 52
    vecs, t = _flow(n, h, w, dev), _target(n, c, h, w, dtype, dev, seed=6)
    g = _upstream((n, c, h, w), dtype, dev).to(memory_format=torch.channels_last)
    assert not g.is_contiguous()
    assert not _is16(_compare(vecs, t, g))
    # padding=: the flow covers a window of the target
    pad = [2, 3, 4, 1]
    tp, gp = _target(n, c, h + 5, w + 5, dtype, dev, seed=7), _upstream((n, c, h + 5, w + 5), dtype, dev)
    res = []
    for native in (True, False):
        v, x = vecs.clone().requires_grad_(True), tp.clone().requires_grad_(True)
        out = ofl.Flow(v, 't').apply(x if native else x.float(), padding=pad, cut=False)
        (out if native else out.to(dtype)).backward(gp)
        if native:
            assert not _is16(_name())
        res.append((x.grad, v.grad))
    _same_bits(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_scaled_source_gradient_is_declined_before_anything_runs(dtype, dev):
    """`warp_bwd_grad_x16` used to hand g_scale to ofl_splat_sum_x16 as its data sign, which takes +-1 only: |g_scale| != 1 with
    want_src raised (status -3) after the flow gradient had been computed.  It is declined up front now, the caller's
    `warp_bwd_grad` scales in fp32; +-1 and the flow gradient alone are still native."""
    from oflibpytorch_amd import _native
    n, c, h, w = 2, 3, 37, 53
    vecs, t, g = _flow(n, h, w, dev), _target(n, c, h, w, dtype, dev, seed=4), _upstream((n, c, h, w), dtype, dev, seed=5)
    assert _native.warp_bwd_grad_x16(vecs, t, g, g_scale=0.5) is None
    assert _native.warp_bwd_grad_x16(vecs, t, g, g_scale=-2.0, want_flow=False) is None
    gs, gf = _native.warp_bwd_grad_x16(vecs, t, g, g_scale=0.5, want_src=False)
    assert gs is None and torch.equal(gf, _native.warp_bwd_grad(vecs, t.float(), g.float(), g_scale=0.5, want_src=False)[1])
    gs, gf = _native.warp_bwd_grad_x16(vecs, t, g, g_scale=-1.0)
    rs, rf = _native.warp_bwd_grad(vecs, t.float(), g.float(), g_scale=-1.0)
    _same_bits(gs, rs.to(dtype), "gradient wrt the target")
    assert torch.equal(gf, rf)


# ---- (7) both families of the flow-gradient launcher -------------------------------------------------------------------
# thresholds in the kernels' 32-wide geometry: g1 = 32 x 16 tiles, g4 = 32 x 64 groups of the launch.  W % 4 == 0: row tables with one
# tile per block below g1 = 5000, four from g4 = 5800, two between; other widths: the four-tile column kernel on the sheared rectangle.
#   (2, ., 96, 136): g1 = 2 * 5 * 6 = 60;   (16, ., 160, 1024): g1 = 16 * 32 * 10 = 5120, g4 = 16 * 32 * 3 = 1536;
#   (46, ., 256, 1024): g4 = 46 * 32 * 4 = 5888
FAMILIES = [((2, 3, 96, 136), r"warp_bwd_rows_kernel<1, 3,"), ((16, 1, 160, 1024), r"warp_bwd_rows_kernel<2, 1,"),
            ((46, 1, 256, 1024), r"warp_bwd_rows_kernel<4, 1,"), ((2, 2, 37, 53), r"warp_bwd_lds_column_kernel<4, 2,"),
            ((2, 3, 96, 134), r"warp_bwd_lds_column_kernel<4, 3,")]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape,kernel", FAMILIES, ids=lambda v: str(v))
def test_both_families_of_the_flow_gradient_launcher(shape, kernel, dtype, dev):
    n, c, h, w = shape
    vecs, t, g = _flow(n, h, w, dev), _target(n, c, h, w, dtype, dev, seed=2), _upstream(shape, dtype, dev, seed=1)
    names = []
    gt, gv = _grads(vecs, t, g, native=True, want=(False, True), names=names)
    rt, rv = _grads(vecs, t, g, native=False, want=(False, True))
    assert re.search(kernel, names[0]) and _is_grad16(names[0], dtype), names[0]
    assert gt is None and rt is None and torch.equal(gv, rv)


# ---- (8) reproducibility -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_two_backward_passes_give_identical_bits(dtype, dev):
    import oflibpytorch_amd as ofl
    n, c, h, w = 2, 5, 96, 136
    vecs, t, g = _flow(n, h, w, dev), _target(n, c, h, w, dtype, dev, seed=3), _upstream((n, c, h, w), dtype, dev, seed=2)
    v, x = vecs.clone().requires_grad_(True), t.clone().requires_grad_(True)
    out = ofl.apply_flow(v, x, 't')
    out.backward(g, retain_graph=True)
    a = (x.grad.clone(), v.grad.clone())
    x.grad = v.grad = None
    out.backward(g)
    b = (x.grad.clone(), v.grad.clone())
    c2 = _grads(vecs, t, g, native=True)                  # ... and on a fresh graph
    for other in (b, c2):
        _same_bits(a[0], other[0])
        assert torch.equal(a[1], other[1])
