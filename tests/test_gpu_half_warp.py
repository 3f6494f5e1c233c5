"""GPU tier: Flow.apply / apply_flow 't' of a feature tensor stored in fp16 / bf16 runs on the 16-bit instantiations of the staged warp
kernels (ofl_warp_bwd_x16) and equals the present fp32 route BIT FOR BIT.

The yardstick everywhere is that route on the same device: the same call on `target.float()`, its result `.to(dtype)` -- what the
reference computes (utils.py:512-618) and what the existing tests pin to the oracle.  Values are compared on their raw 16-bit
patterns, masks and valid areas as bool.  After every case the name the library reports for the launch must be a 16-bit
instantiation; the last test holds the set of names seen against the list of every instantiation the launcher can pick."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
SEEN = set()          # demangled names of the 16-bit kernels the cases of this file reached

# every instantiation warp_choose() can pick for x16_launch / x16_launch_group (ofl_kernels.hip, OFL_X16_TU), as (family, tiles per block, planes, VALID)
ROWS = [("rows", t, nc, v) for t in (1, 2, 4) for nc in (1, 2, 3) for v in (True, False)]            # W % 4 == 0: row tables
COLUMN = [("column", t, nc, v) for t in (1, 4) for nc in (1, 2, 3) for v in (True, False)]           # other widths: one tile / four-tile columns
PAIR = [("pair", 2, nc, v) for nc in (1, 2, 3) for v in (True, False)]                               # ... and the two-tile kernel between them
CHAN = [("chan_rows", 1, 0, True), ("chan_rows", 1, 0, False), ("chan", 1, 0, False)]                # more than 3 planes: the channel loop
EXPECTED = {(k, dt) for k in ROWS + COLUMN + PAIR + CHAN for dt in DTYPES}

# frames (H, W) that put a launch of ONE image into each size class of the launcher.  Its thresholds count 32 x 16 tiles (g1) and groups
# of four of them, 32 x 64 (g4): row tables -- 1 tile per block below g1 = 5000 (OFL_ROWS_T1_MAX), 4 from g4 = 5800 (OFL_ROWS_T4_MIN), 2
# between; other widths -- one tile below g1 = 6912 (kColumnMinGroups), four-tile columns from g4 = 6912, the pair kernel between.
#   2048 x 2048: g1 = 64 * 128 = 8192, g4 = 64 * 32 = 2048;   3456 x 4096: g4 = 128 * 54 = 6912 (the same counts at widths 2046 / 4094)
SIZE = {("rows", 1): (96, 136), ("rows", 2): (2048, 2048), ("rows", 4): (3456, 4096),
        ("column", 1): (37, 53), ("pair", 2): (2048, 2046), ("column", 4): (3456, 4094)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tier needs a HIP device"
    from oflibpytorch_amd import _native
    _native.load_library()
    return torch.device('cuda', 0)


def _key(name):
    """(family, tiles, planes, VALID), dtype of a demangled kernel name -- None for a kernel on fp32 planes."""
    dt = torch.float16 if "half_t" in name else torch.bfloat16 if "bf16_t" in name else None
    if dt is None:
        return None
    b = lambda s: s == "true"
    m = re.search(r"warp_bwd_rows_kernel<(\d+), (\d+), (true|false),", name)
    if m:
        return ("rows", int(m.group(1)), int(m.group(2)), b(m.group(3))), dt
    m = re.search(r"warp_bwd_lds_column_kernel<(\d+), (\d+), (true|false),", name)
    if m:
        return ("column", int(m.group(1)), int(m.group(2)), b(m.group(3))), dt
    m = re.search(r"warp_bwd_lds_kernel<(\d+), (true|false),", name)
    if m:
        return ("pair", 2, int(m.group(1)), b(m.group(2))), dt
    m = re.search(r"warp_bwd_lds_chan_kernel<(true|false), true, 1, (true|false),", name)
    if m:
        return ("chan_rows" if b(m.group(2)) else "chan", 1, 0, b(m.group(1))), dt
    raise AssertionError("a 16-bit kernel this file does not know: " + name)


def _note(dtype):
    from oflibpytorch_amd import _native
    name = _native.last_kernel_name()
    key = _key(name)
    assert key is not None and key[1] == dtype, "not a %s instantiation: %s" % (dtype, name)
    SEEN.add(key)
    return key[0][0]                # the family


_FLOWS = {}


def _flow(n, h, w, dev):
    """sigma ~ 4 smooth random flow with an exactly-zero disc and two corner blocks whose displacements leave the frame (cached)."""
    if (n, h, w) not in _FLOWS:
        g = torch.Generator().manual_seed(1000 * n + h + w)
        lo = (torch.randn(n, 2, max(h // 12, 2), max(w // 12, 2), generator=g) * 4).to(dev)
        f = torch.nn.functional.interpolate(lo, size=(h, w), mode='bicubic', align_corners=True).contiguous()
        yy, xx = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing='ij')
        f[:, :, (yy - h // 2) ** 2 + (xx - w // 3) ** 2 < (min(h, w) // 6) ** 2] = 0.0
        f[:, :, :6, :6] = 30.0
        f[:, :, -6:, -6:] = -30.0
        _FLOWS[(n, h, w)] = f
    return _FLOWS[(n, h, w)]


def _target(n, c, h, w, dtype, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(7 + seed)
    return (torch.randn(n, c, h, w, generator=g, device=dev) * 3).to(dtype)


def _holes(n, h, w, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.rand(n, h, w, generator=g, device=dev) > 0.2


def _same_bits(got, ref, what=""):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    assert torch.equal(got.contiguous().view(torch.int16), ref.contiguous().view(torch.int16)), what


def _apply_both(vecs, target, *, flow_mask=None, target_mask=None, valid=False):
    """Flow.apply on the 16-bit target, the name of the kernel it ran, and the present route's result."""
    import oflibpytorch_amd as ofl
    f = ofl.Flow(vecs, 't', flow_mask)
    kw = dict(target_mask=target_mask, return_valid_area=valid) if valid else {}
    got = f.apply(target, **kw)
    fam = _note(target.dtype)
    ref = f.apply(target.float(), **kw)
    if valid:
        assert got[1].dtype == torch.bool and torch.equal(got[1], ref[1])
        got, ref = got[0], ref[0]
    assert ref.dtype == torch.float32
    _same_bits(got, ref.to(target.dtype))
    return fam


# ---- (1) bit-exact values ----------------------------------------------------------------------------------------------
# the large frame passes kColumnMinGroups = 6912 four-tile groups of 32 x 64 pixels with B = 2: 2 * (4096 / 32) * (1728 / 64) = 6912
SHAPES = [(3, 4, 37, 53), (2, 3, 96, 136), (2, 1, 96, 136), (1, 64, 64, 96), (2, 5, 270, 480), (2, 1, 1728, 4096)]
FAMILY = {(3, 4, 37, 53): "column", (2, 3, 96, 136): "rows", (2, 1, 96, 136): "rows", (1, 64, 64, 96): "chan_rows",
          (2, 5, 270, 480): None, (2, 1, 1728, 4096): "rows"}          # (5 planes: the channel loop, or 3 + 2 with the valid area)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_16_bit_targets_equal_the_fp32_route_bit_for_bit(shape, dtype, dev):
    import oflibpytorch_amd as ofl
    n, c, h, w = shape
    nb = max(n, 2)                                           # (the B = 1 shape still broadcasts: over a flow / data batch of 2)
    vecs, t = _flow(nb, h, w, dev), _target(nb, c, h, w, dtype, dev)
    tm, fm = _holes(nb, h, w, dev, 1), _holes(nb, h, w, dev, 2)
    fams = set()
    # plain, through apply_flow (the function) and through Flow.apply
    got = ofl.apply_flow(vecs[:n], t[:n], 't')
    fams.add(_note(dtype))
    _same_bits(got, ofl.apply_flow(vecs[:n], t[:n].float(), 't').to(dtype))
    fams.add(_apply_both(vecs[:n], t[:n]))
    # flow batch 1 under data batch N, and the reverse
    got = ofl.apply_flow(vecs[:1], t, 't')
    fams.add(_note(dtype))
    _same_bits(got, ofl.apply_flow(vecs[:1], t.float(), 't').to(dtype))
    fams.add(_apply_both(vecs, t[:1], valid=True))
    # the valid area: without and with the target mask, with a flow mask with holes
    fams.add(_apply_both(vecs[:n], t[:n], valid=True))
    fams.add(_apply_both(vecs[:n], t[:n], target_mask=tm[:n], valid=True))
    fams.add(_apply_both(vecs[:n], t[:n], flow_mask=fm[:n], valid=True))
    fams.add(_apply_both(vecs[:n], t[:n], flow_mask=fm[:n], target_mask=tm[:n], valid=True))
    if FAMILY[shape] is not None:
        assert fams == {FAMILY[shape]}, fams
    else:
        assert fams == {"chan", "rows"}, fams


CLASSES = sorted(SIZE)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("cls", CLASSES, ids=str)
def test_every_size_class_and_plane_count_equals_the_fp32_route(cls, dtype, dev):
    """1, 2 and 3 planes, with and without the valid area, in each size class of the launcher (a batch-1 frame sized for the class): the
    six instantiations of the class's kernel."""
    h, w = SIZE[cls]
    vecs, t3, tm = _flow(1, h, w, dev), _target(1, 3, h, w, dtype, dev, seed=1), _holes(1, h, w, dev, 3)
    for c in (1, 2, 3):
        t = t3[:, :c].contiguous()
        assert _apply_both(vecs, t) == cls[0]
        assert _apply_both(vecs, t, target_mask=tm, flow_mask=tm, valid=True) == cls[0]
    assert {(cls[0], cls[1], c, v) for c in (1, 2, 3) for v in (True, False)} <= {k for k, d in SEEN if d == dtype}


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_channel_loop_instantiations(dtype, dev):
    h, w = 64, 96
    vecs, t, tm = _flow(2, h, w, dev), _target(2, 9, h, w, dtype, dev, seed=2), _holes(2, h, w, dev, 4)
    assert _apply_both(vecs, t) == "chan_rows"                                            # 9 planes: groups 4 + 4 + the last one again from plane 5
    assert _apply_both(vecs, t, target_mask=tm, valid=True) == "chan_rows"                # 3 + mask, then 4 + 4 (the last from plane 5)
    assert _apply_both(vecs, t[:, :4].contiguous()) == "chan"                             # one group: no row tables
    assert _apply_both(vecs, t[:, :6].contiguous()) == "chan"


# ---- (2) rounding ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_results_on_and_next_to_rounding_ties(dtype, dev):
    """Data with every mantissa bit of the format in use (integers in [2^(p-1), 2^p), p = 8 / 11 significant bits) under displacements
    of exactly 0.5 and 0.25 px: the fp32 blends need one / two more bits than the format holds -- exact ties and their neighbours."""
    n, c, h, w = 2, 3, 40, 52
    p = 8 if dtype == torch.bfloat16 else 11
    g = torch.Generator(device=dev).manual_seed(11)
    t = torch.randint(2 ** (p - 1), 2 ** p, (n, c, h, w), generator=g, device=dev).to(dtype)
    assert torch.equal(t.float().to(dtype), t)
    t[:, 1] = -t[:, 1]
    t[:, 2] = t[:, 2] / 64
    vecs = torch.zeros(n, 2, h, w, device=dev)
    vecs[:, 0, :, : w // 2] = 0.5
    vecs[:, 0, :, w // 2:] = 0.25
    vecs[:, 1, h // 2:] = 0.5
    vecs[1] = -vecs[1]
    assert _apply_both(vecs, t) == "rows"
    assert _apply_both(vecs, t, valid=True) == "rows"
    # and on the channel loop's store
    assert _apply_both(vecs, torch.cat((t, t.flip(1), t), dim=1)) == "chan_rows"


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_nan_and_infinities_come_out_as_tensor_to_gives_them(dtype, dev):
    import oflibpytorch_amd as ofl
    n, c, h, w = 2, 3, 40, 52
    t = _target(n, c, h, w, dtype, dev, seed=5)
    t[0, 0, 5:9, 7:11] = float('nan')
    t[0, 1, 20, 30] = float('inf')
    t[1, 2, 11, 12:20] = float('-inf')
    t[1, 0, 30, 40] = float('inf')
    t[1, 0, 30, 41] = float('-inf')                       # (inf next to -inf: a NaN where both are blended)
    t[0, 2, 3, 3] = torch.finfo(dtype).max                # (finite, and stays finite or overflows exactly as the conversion does)
    vecs = _flow(n, h, w, dev)
    got = ofl.apply_flow(vecs, t, 't')
    assert _note(dtype) == "rows"
    ref = ofl.apply_flow(vecs, t.float(), 't').to(dtype)
    nan = torch.isnan(ref)
    assert nan.any() and torch.isinf(ref).any() and torch.equal(torch.isnan(got), nan)
    assert torch.equal(got.view(torch.int16)[~nan], ref.view(torch.int16)[~nan])
    assert torch.allclose(got.float(), ref.float(), rtol=0, atol=0, equal_nan=True)


# ---- (3) no fp32 copy --------------------------------------------------------------------------------------------------
def test_no_fp32_copy_of_the_target_is_made(dev):
    """Peak memory of one apply_flow call above the level before it: the 16-bit result (target.numel() * 2 bytes) and flow-sized
    by-products -- bounded by 1.5 x the result plus one fp32 flow.  The copy route needs the fp32 target and the fp32 result at once:
    at least target.numel() * 8 bytes, 2.6 x the bound at this shape."""
    import oflibpytorch_amd as ofl
    n, c, h, w = 2, 32, 270, 480
    vecs, t = _flow(n, h, w, dev), _target(n, c, h, w, torch.bfloat16, dev)
    bound = 1.5 * t.numel() * 2 + vecs.numel() * 4
    assert bound < t.numel() * 8
    ofl.apply_flow(vecs, t, 't')                          # (warm: host words, the library's own first-call allocations)
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    out = ofl.apply_flow(vecs, t, 't')
    torch.cuda.synchronize(dev)
    peak = torch.cuda.max_memory_allocated(dev) - before
    assert _note(torch.bfloat16) == "chan_rows"
    assert out.dtype == torch.bfloat16
    assert peak < bound, "peak %d bytes above the level before the call; bound %d, fp32 copies need %d" % (peak, bound, t.numel() * 8)


# ---- (4) autograd ------------------------------------------------------------------------------------------------------
def _warp_node(out):
    todo, seen = [out.grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if "WarpFn" in type(fn).__name__:
            return fn
        todo.extend(f for f, _ in fn.next_functions)
    raise AssertionError("no WarpFn node in the graph")


@pytest.mark.parametrize("shape", [(2, 6, 37, 53), (1, 4, 96, 136)], ids=str)
def test_autograd_saves_the_16_bit_source_and_gives_the_fp32_routes_gradients(shape, dev):
    """Forward on the native 16-bit launch; WarpFn keeps the bf16 source (not an fp32 copy) for the backward; the backward kernels see
    the same fp32 values as on the present route (exact up-conversion of the same source, the same upstream gradient), so the gradients
    are compared exactly: wrt the target in bf16, wrt the flow in fp32."""
    import oflibpytorch_amd as ofl
    n, c, h, w = shape
    dtype = torch.bfloat16
    vecs, t = _flow(n, h, w, dev), _target(n, c, h, w, dtype, dev, seed=9)
    plain = ofl.apply_flow(vecs, t, 't')
    v1, t1 = vecs.clone().requires_grad_(True), t.clone().requires_grad_(True)
    out = ofl.apply_flow(v1, t1, 't')
    fam = _note(dtype)
    assert fam == ("column" if w % 4 else "chan")
    assert out.dtype == dtype and out.requires_grad
    _same_bits(out.detach(), plain)
    _same_bits(plain, ofl.apply_flow(vecs, t.float(), 't').to(dtype))
    saved = _warp_node(out).saved_tensors
    assert saved[1].dtype == dtype and saved[1].shape == t.shape, "WarpFn saved %s for the source" % saved[1].dtype
    g = torch.randn(out.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(3)).to(dtype)
    out.backward(g)
    v2, t2 = vecs.clone().requires_grad_(True), t.clone().requires_grad_(True)
    ofl.apply_flow(v2, t2.float(), 't').to(dtype).backward(g)
    assert t1.grad.dtype == dtype and v1.grad.dtype == torch.float32
    _same_bits(t1.grad, t2.grad, "gradient wrt the target")
    assert torch.equal(v1.grad, v2.grad), "gradient wrt the flow"


# ---- (5) unchanged routes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_other_routes_are_unchanged(dtype, dev):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _native
    n, c, h, w = 2, 3, 40, 52
    vecs, t = _flow(n, h, w, dev), _target(n, c, h, w, dtype, dev, seed=6)
    fp32_kernel = lambda: _key(_native.last_kernel_name()) is None
    # padding=: the flow is read through a window by the generic fp32 kernel
    pad = [2, 3, 4, 1]
    tp = _target(n, c, h + 5, w + 5, dtype, dev, seed=7)
    got = ofl.Flow(vecs, 't').apply(tp, padding=pad, cut=False)
    assert fp32_kernel() and got.dtype == dtype
    _same_bits(got, ofl.Flow(vecs, 't').apply(tp.float(), padding=pad, cut=False).to(dtype))
    # an 's' flow: the splat
    got = ofl.apply_flow(vecs, t, 's')
    assert fp32_kernel() and got.dtype == dtype
    _same_bits(got, ofl.apply_flow(vecs, t.float(), 's').to(dtype))
    # an all-zero flow: the target itself
    z = torch.zeros_like(vecs)
    assert ofl.apply_flow(z, t, 't') is t
    got = ofl.Flow(z, 't').apply(t)
    assert got.dtype == dtype and torch.equal(got, t)
    # a CPU tensor with 16-bit data is staged through the device as fp32
    got = ofl.apply_flow(vecs.cpu(), t.cpu(), 't')
    assert fp32_kernel() and got.dtype == dtype and got.device.type == 'cpu'
    _same_bits(got, ofl.apply_flow(vecs, t.float(), 't').to(dtype).cpu())
    # a Flow as the target stays fp32 (fp16-stored flows included)
    res = ofl.Flow(vecs, 't').apply(ofl.Flow(vecs * 0.5, 't'))
    assert fp32_kernel() and res.vecs.dtype == torch.float32


# ---- the whole file ----------------------------------------------------------------------------------------------------
def test_zz_every_16_bit_instantiation_was_reached():
    """(runs last in this file) every kernel the 16-bit launcher can pick has run, and been compared, in the cases above"""
    assert len(EXPECTED) == 2 * (18 + 12 + 6 + 3)
    missing = sorted(map(str, EXPECTED - SEEN))
    assert not missing, "16-bit instantiations no case reached: %s" % missing
    assert SEEN <= EXPECTED, sorted(map(str, SEEN - EXPECTED))
