"""GPU tier: every primitive of `oflibpytorch_amd._native` on dirty, guarded memory (tests/dirty_memory.py).

One parametrised test over CASES.  A case names the `_native` function whose allocations it is about (`primitive`, plus declared
`callees` that allocate on its behalf), builds its inputs on the CPU from the generators the oracle-pinned tests use, and runs once per
fill byte (0x00, 0xFF, 0x55) with every `torch.empty` / `torch.zeros` of `_native` served by the harness and every input copied into a
guarded buffer.  The test asserts:

1. same bits under every fill: every returned tensor of the 0xFF and 0x55 runs equals the 0x00 run byte for byte (`view(torch.uint8)`:
   NaN payloads and bool bytes count); bool outputs (and the uint8 outputs a case declares `boolish`) hold only the bytes 0 and 1;
2. the control is the pinned result: the 0x00 run is compared with the oracle / second route of the case's existing test, under that
   test's bar (`control`);
3. no stray write, no written input: `check_guards()` and `check_inputs_unchanged()` after every run;
4. the harness was in the path: the log of every run is non-empty and its calling functions include `primitive`.

Atomic exception list
---------------------
Only where float atomics write the compared output may the bits differ between runs.  Such a case has an `atomic` bar: under EACH fill
its float outputs are held to the bar of its existing test against that test's reference (never to the 0x00 run), may hold no
non-finite value where the reference has none, and everything else it returns (masks, flag words, outputs no atomic writes) is still
compared byte for byte.  The cases, by id prefix, with the kernel and the line of the atomic:

  splat.fold                      LDS float atomics of a fold band   sp_tile_atomics            ofl_kernels.hip:2826
  splat.list_limit                LDS float atomics of a fold band   sp_tile_atomics            ofl_kernels.hip:2826
  splat.queue_capacity            global two-pass path (per image)   splat_fwd_tiles            ofl_kernels.hip:1981
  splat.fallback_slots            global two-pass path (per image)   splat_fwd_tiles            ofl_kernels.hip:1981
  splat.passes_rough              global two-pass path (per image)   splat_fwd_tiles            ofl_kernels.hip:1981
  splat.narrow                    global two-pass path (W < 4)       splat_fwd_tiles            ofl_kernels.hip:1981
  splat.two_pass                  global two-pass path (forced)      splat_fwd_tiles            ofl_kernels.hip:1981
  grad.warp-2x9x3                 grad_src of ofl_warp_bwd_grad_f32  warp_grad_kernel           ofl_aux_kernels.hip:99
  grad.pts                        grad_flow of ofl_sample_pts_grad   sample_pts_kernel<true>    ofl_aux_kernels.hip:315

(The W < 4 frame of `grad.splat` stays bit for bit: its `out` / `density` inputs come from one forward made before the fills, and
splat_grad_kernel gathers.)  tests/test_dirty_memory_host.py checks that every prefix above names a case and that every allocation
site of `_native.py` is the primitive or a declared callee of some case.

Importing this module touches no device: builders run inside the test.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

import dirty_memory as dm
import grad_cases64 as gc

pytestmark = pytest.mark.gpu

CL = torch.channels_last
ATOMIC_EXCEPTIONS = {
    "splat.fold": ("sp_tile_atomics", "ofl_kernels.hip:2826"),
    "splat.list_limit": ("sp_tile_atomics", "ofl_kernels.hip:2826"),
    "splat.queue_capacity": ("splat_fwd_tiles", "ofl_kernels.hip:1981"),
    "splat.fallback_slots": ("splat_fwd_tiles", "ofl_kernels.hip:1981"),
    "splat.passes_rough": ("splat_fwd_tiles", "ofl_kernels.hip:1981"),
    "splat.narrow": ("splat_fwd_tiles", "ofl_kernels.hip:1981"),
    "splat.two_pass": ("splat_fwd_tiles", "ofl_kernels.hip:1981"),
    "grad.warp-2x9x3": ("warp_grad_kernel", "ofl_aux_kernels.hip:99"),
    "grad.pts": ("sample_pts_kernel<true>", "ofl_aux_kernels.hip:315"),
}


class Case(object):
    """id; primitive (the `_native` function that allocates; a tuple for a Flow-level chain: at least one of them must); build() -> {name: CPU tensor | None | value}; run(nat, ofl, g) with g
    the same dict on the device, tensors guarded -> result; control(res0, inp) on the 0x00 run; atomic(res, inp, res0) under each fill
    (exception list only); options() a context manager that sets and restores library options; boolish: indices of the flattened
    result that are uint8 outputs holding booleans."""

    def __init__(self, id, primitive, build, run, callees=(), control=None, atomic=None, options=None, boolish=(), prepare=None):
        self.id, self.primitive, self.build, self.run = id, primitive, build, run
        self.callees, self.control, self.atomic, self.options, self.boolish = tuple(callees), control, atomic, options, tuple(boolish)
        self.prepare = prepare     # prepare(nat, ofl, device inputs) -> more inputs, made ONCE before the fills with real allocations
        self.side = {}


CASES = []


def case(*a, **kw):
    CASES.append(Case(*a, **kw))


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _eq_bits(got, want, what):
    """NumPy arrays: same dtype, shape and bytes."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = got.view(np.uint8) != want.view(np.uint8)
    assert not bad.any(), "%s: %d bytes differ from the reference" % (what, int(bad.sum()))


def _eq_values(got, want, what):
    """Equal as numbers (NaN == NaN, -0.0 == +0.0): the bar of the tests that use np.array_equal(..., equal_nan=True)."""
    assert got.shape == want.shape, what
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == 'f'), "%s: %d elements differ" % (
        what, int((~((got == want) | ((got != got) & (want != want)))).sum()))


def _finite_where_ref(got, ref, what):
    bad = ~np.isfinite(got) & np.isfinite(ref)
    assert not bad.any(), "%s: %d non-finite values where the reference is finite" % (what, int(bad.sum()))


def _smooth(n, h, w, sigma, seed):
    """tests/test_gpu_parity.py::_smooth, on the CPU"""
    g = torch.Generator().manual_seed(seed)
    lo = torch.randn(n, 2, max(h // 12, 2), max(w // 12, 2), generator=g) * sigma
    return torch.nn.functional.interpolate(lo, size=(h, w), mode='bicubic', align_corners=True).contiguous()


@contextlib.contextmanager
def _option(setter, value, restore=0):
    from oflibpytorch_amd import _native
    fn = getattr(_native, setter)
    fn(value)
    try:
        yield
    finally:
        fn(restore)


@contextlib.contextmanager
def _splat_stats(level=True):
    from oflibpytorch_amd import _native
    old = _native.collect_splat_stats
    _native.collect_splat_stats = level
    try:
        yield
    finally:
        _native.collect_splat_stats = old
        _native._last_splat_ws = None


# ==================================================================================================================================
# backward warp
# ==================================================================================================================================
def _choice_cases():
    """tests/golden/warp_kernel_choice.json: per distinct recorded kernel name the case of cases() with the smallest n * h * w."""
    import test_gpu_warp_kernel_choice as wk
    best = {}
    for c in wk.CASES:
        name, size = wk.RECORDED[c["id"]], c["n"] * c["h"] * c["w"]
        if name not in best or (size, c["id"]) < best[name][0]:
            best[name] = ((size, c["id"]), c)
    return [c for _, c in sorted(best.values(), key=lambda v: (v[1]["n"], v[1]["h"], v[1]["w"], v[1]["id"]))]


def _choice_primitive(c):
    if c["kind"] == "grad":
        return "warp_bwd_grad"
    if c["kind"] == "half":
        return "_warp_bwd_half_src"
    if c["kind"] == "u8" or c.get("flags") or c.get("dst_flags") or c.get("src_b"):
        return "_warp_bwd_raw"
    return "_warp_bwd_lean"


def _add_choice(c):
    import test_gpu_warp_kernel_choice as wk
    key = (c["n"], c["h"], c["w"])

    def build():
        return {}

    def prepare(nat, ofl, g):
        dev = torch.device('cuda', 0)
        return {"data": wk._data(c, dev)}                   # (flow, planes, other, mask) on the device, from the test's own generator

    def run(nat, ofl, g):
        dev = torch.device('cuda', 0)
        keep = wk._DATA.get(key)
        wk._DATA[key] = tuple(g["data"])                     # the guarded copies, for this run only
        try:
            res, name = wk.run_case(c, dev)
        finally:
            if keep is None:
                wk._DATA.pop(key, None)
            else:
                wk._DATA[key] = keep
        assert name == wk.RECORDED[c["id"]], name
        return res

    def control(res0, inp):
        dev = torch.device('cuda', 0)
        ref = wk._second_route(c, dev)                       # the existing test's bar: torch.equal with the second route
        a, b = dm.flatten(res0), dm.flatten(ref)
        assert len(a) == len(b)
        for k, (x, y) in enumerate(zip(a, b)):
            assert (x is None) == (y is None)
            if x is not None:
                assert x.dtype == y.dtype and torch.equal(x, y), "result %d differs from the second route" % k
        if c["kind"] == "plain" and not c.get("addend") and not c.get("src_b") and c["n"] * c["h"] * c["w"] <= 300000:
            from oracle import oracle                        # (and the oracle where the batch is small: test_gpu_parity.py's bar)
            flow, planes, other, mask = (t.cpu() for t in wk._data(c, dev))
            src = planes[:, :c["c"]].numpy()
            if c.get("valid"):
                src = np.concatenate([src, mask.numpy()[:, None].astype(np.float32)], 1)
            gref = oracle.G(flow.numpy(), np.ascontiguousarray(src))
            _eq_values(_np(res0[0]), gref[:, :c["c"]], "dst against oracle.G")
            if c.get("valid"):
                assert np.array_equal(_np(res0[1]), oracle.theta(gref[:, c["c"]]) & mask.numpy())

    case("warp.choice." + c["id"], _choice_primitive(c), build, run, control=control, prepare=prepare)


for _c in _choice_cases():
    _add_choice(_c)


def _warp_inputs(n, c, h, w, seed, kind="smooth", masks=True, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    flow = _smooth(n, h, w, 3.0, seed + 1)
    flow[:, :, : max(h // 5, 1), : max(w // 5, 1)] = 40.0            # taps that leave the frame
    if kind == "outside":                                             # every tap outside the frame
        flow = torch.stack([torch.full((n, h, w), 3.0 * w + 7.3), torch.full((n, h, w), -(3.0 * h + 5.1))], 1).contiguous()
    src = (torch.randn(n, c, h, w, generator=g) * 3).to(dtype)
    out = dict(flow=flow, src=src, sm=None, fm=None)
    if masks:
        out["sm"] = torch.rand(n, h, w, generator=g) > 0.2
        out["fm"] = torch.rand(n, h, w, generator=g) > 0.2
    return out


def _oracle_warp(inp, want_valid, **kw):
    import oracle_backend as ob
    return ob.warp_bwd(inp["flow"], inp["src"].float(), src_mask=inp["sm"], flow_mask=inp["fm"], want_valid=want_valid, **kw)


def _add_outside(shape, want_valid):
    n, c, h, w = shape

    def run(nat, ofl, g):
        return nat.warp_bwd(g["flow"], g["src"], src_mask=g["sm"], flow_mask=g["fm"], want_valid=want_valid)[:2]

    def control(res0, inp):
        assert not _np(res0[0]).view(np.uint32).any(), "dst is not all +0.0"
        if want_valid:
            assert not _np(res0[1]).view(np.uint8).any()
        ref = _oracle_warp(inp, want_valid)
        _eq_values(_np(res0[0]), _np(ref[0]), "dst")

    case("warp.outside-%dx%dx%dx%d-valid%d" % (n, c, h, w, want_valid), "_warp_bwd_lean",
         functools.partial(_warp_inputs, n, c, h, w, 11, "outside", want_valid), run, control=control)


for _shape in [(2, 3, 9, 3), (1, 3, 2, 8), (1, 2, 37, 52), (2, 3, 45, 97), (3, 2, 130, 260)]:
    for _v in (True, False):
        _add_outside(_shape, _v)


def _add_win(shape, pad):
    n, c, hp, wp = shape
    h, w = hp - pad[0] - pad[1], wp - pad[2] - pad[3]

    def build():
        g = torch.Generator().manual_seed(21)
        f = _smooth(n, h, w, 3.0, 5)
        f[0, :, : h // 4] = 0
        return dict(flow=f, fm=torch.rand(n, h, w, generator=g) > 0.15, src=torch.rand(n, c, hp, wp, generator=g) * 200,
                    sm=torch.rand(n, hp, wp, generator=g) > 0.1)

    def run(nat, ofl, g):
        return nat.warp_bwd_win(g["flow"], g["src"], (pad[0], pad[2]), src_mask=g["sm"], flow_mask=g["fm"], want_valid=True)

    def control(res0, inp):
        import oracle_backend as ob
        ref = ob.warp_bwd_win(inp["flow"], inp["src"], (pad[0], pad[2]), src_mask=inp["sm"], flow_mask=inp["fm"], want_valid=True)
        _eq_values(_np(res0[0]), _np(ref[0]), "dst")
        assert np.array_equal(_np(res0[1]), _np(ref[1]))

    case("warp.win-%dx%dx%dx%d" % shape, "warp_bwd_win", build, run, control=control)


PADS = [((2, 3, 70, 132), [3, 5, 4, 2]), ((1, 2, 40, 61), [0, 7, 9, 0]), ((3, 1, 33, 47), [6, 0, 0, 5]), ((2, 3, 150, 260), [11, 13, 17, 19])]
for _shape, _pad in PADS:
    _add_win(_shape, _pad)


def _add_x16(shape, dtype):
    n, c, h, w = shape

    def run(nat, ofl, g):
        res = nat.warp_bwd_keep16(g["flow"], g["src"], src_mask=g["sm"], flow_mask=g["fm"], want_valid=True)
        assert res is not None, "ofl_warp_bwd_x16 declined the launch"
        return res[:2]

    def control(res0, inp):
        ref = _oracle_warp(inp, True)                         # the fp32 result rounded once (tests/test_gpu_half_warp.py's bar)
        assert res0[0].dtype == dtype
        _eq_bits(_np(res0[0].view(torch.int16)), _np(ref[0].to(dtype).view(torch.int16)), "dst")
        assert np.array_equal(_np(res0[1]), _np(ref[1]))

    case("warp.x16-%s-%dx%dx%dx%d" % ((str(dtype).split(".")[1],) + shape), "_warp_bwd_x16",
         functools.partial(_warp_inputs, n, c, h, w, 31, "smooth", True, dtype), run, control=control)


for _dtype in (torch.float16, torch.bfloat16):
    for _shape in [(3, 4, 37, 53), (2, 3, 96, 136), (1, 64, 64, 96)]:
        _add_x16(_shape, _dtype)


def _add_nhwc(shape, dtype):
    n, c, h, w = shape
    native = c % 4 == 0

    def build():
        inp = _warp_inputs(n, c, h, w, 41, "smooth", True, dtype)
        inp["src"] = inp["src"].contiguous(memory_format=CL)
        return inp

    def run(nat, ofl, g):
        assert g["src"].is_contiguous(memory_format=CL) and not g["src"].is_contiguous()
        res = nat.warp_bwd_nhwc(g["flow"], g["src"], src_mask=g["sm"], flow_mask=g["fm"], want_valid=True)
        assert (res is not None) == native, "C = %d: %s" % (c, "declined" if native else "not declined")
        if res is None:                                       # C no multiple of 4: the planar route, cleanly
            res = nat.warp_bwd(g["flow"], g["src"], src_mask=g["sm"], flow_mask=g["fm"], want_valid=True)
            assert res[0].is_contiguous()
        else:
            assert res[0].is_contiguous(memory_format=CL)
        return res[:2]

    def control(res0, inp):
        ref = _oracle_warp(inp, True)
        if dtype == torch.float32:
            _eq_values(_np(res0[0]), _np(ref[0]), "dst")
        else:
            _eq_bits(_np(res0[0].contiguous().view(torch.int16)), _np(ref[0].to(dtype).view(torch.int16)), "dst")
        assert np.array_equal(_np(res0[1]), _np(ref[1]))

    case("warp.nhwc-%s-%dx%dx%dx%d" % ((str(dtype).split(".")[1],) + shape), "_warp_bwd_nhwc" if native else "_warp_bwd_raw", build, run,
         control=control)


for _shape, _dtype in [((2, 4, 37, 53), torch.float32), ((2, 8, 33, 47), torch.float32), ((2, 8, 37, 53), torch.float16),
                       ((2, 6, 37, 53), torch.float32)]:
    _add_nhwc(_shape, _dtype)


# ==================================================================================================================================
# gather splat
# ==================================================================================================================================
def _oracle_splat(inp, **kw):
    import oracle_backend as ob
    names = dict(wm="weight_mask", ca="chan_mask_a", cb="chan_mask_b", xs="xs", ys="ys", data_b="data_b")
    kw.update({names[k]: v for k, v in inp.items() if k in names and v is not None})
    return ob.splat_fwd(inp.get("flow"), inp["data"].float(), **kw)


def _splat_kw(g):
    names = dict(wm="weight_mask", ca="chan_mask_a", cb="chan_mask_b", xs="xs", ys="ys", data_b="data_b")
    return {names[k]: v for k, v in g.items() if k in names and v is not None}


def _exact_splat_control(kw):
    def control(res0, inp):
        ref = _oracle_splat(inp, **kw)
        for k, (a, b) in enumerate(zip(res0, ref)):
            assert (a is None) == (b is None), k
            if a is not None:
                _eq_values(_np(a), _np(b), "splat result %d" % k)
    return control


def _bars_splat(kw, rtol, atol_v, atol_den, atol_m=None, exact_images=()):
    """The bar of a splat whose values float atomics write: masks and flag words exact, values / density / mask channel within
    the existing test's tolerances against the oracle, no non-finite value where the oracle has none; `exact_images` bit for bit."""
    def atomic(res, inp, res0):
        ref = _oracle_splat(inp, **kw)
        for k, (a, b) in enumerate(zip(res, ref)):
            assert (a is None) == (b is None), k
            if a is None:
                continue
            a, b = _np(a), _np(b)
            if a.dtype.kind != 'f':
                assert np.array_equal(a, b), "splat result %d (%s) differs from the oracle" % (k, a.dtype)
                continue
            _finite_where_ref(a, b, "splat result %d" % k)
            atol = atol_v if k == 0 else (atol_den if k == 2 else (atol_m if atol_m is not None else atol_v))
            np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg="splat result %d" % k)
            if k == 1 and kw.get("want_mask_chan"):
                assert np.array_equal(a == 1, b == 1)
            for i in exact_images:
                _eq_values(a[i], b[i], "splat result %d, in-order image %d" % (k, i))
    return atomic


def _cells_inputs(kind, c, holes, half=False):
    import splat_cells as sc
    fr, info, data, ca = sc.make(kind)
    f, d = torch.from_numpy(fr.flow.copy()), torch.from_numpy(np.ascontiguousarray(data[:, :c]))
    if half:
        f, d = f.half(), d.half()
    return dict(flow=f, data=d, wm=torch.from_numpy(fr.on.copy()), ca=torch.from_numpy(ca.copy()) if holes else None)


def _add_cells(kind, c, holes, occlude=True):
    kw = dict(occlude=occlude, want_density=True, want_warped=True)
    if holes:
        kw["want_mask_chan"] = True

    def run(nat, ofl, g):
        return nat.splat_fwd(g["flow"], g["data"], **dict(kw, **_splat_kw(g)))

    case("splat.cells-%s-c%d-holes%d" % (kind, c, holes), "_splat_fwd_raw", functools.partial(_cells_inputs, kind, c, holes), run,
         callees=("_fallback_accum",), control=_exact_splat_control(kw))


for _kind in ("first", "second"):
    _add_cells(_kind, 3, True)
    _add_cells(_kind, 2, False, occlude=False)
_add_cells("first", 5, True)                                  # channel groups of 3: the redo list is filled anew per group


def _add_fold(c, holes):
    """splat_cells.fold_frame: the marked bands add with LDS float atomics; every pixel outside them stays bit for bit the oracle's
    (tests/test_gpu_splat_cells.py::test_folds_stay_inside_the_marked_bands and its bars)."""
    import splat_cells as sc
    kw = dict(occlude=True, want_density=True, want_warped=True)
    if holes:
        kw["want_mask_chan"] = True
    this = []

    def run(nat, ofl, g):
        res = nat.splat_fwd(g["flow"], g["data"], **dict(kw, **_splat_kw(g)))
        this[0].side["ws"] = nat._last_splat_ws.cpu().numpy()
        this[0].side["stats"] = nat._last_splat_stats.cpu().tolist()
        return res

    def atomic(res, inp, res0):
        from oflibpytorch_amd import _native
        fr = sc.make("fold")[0]
        units = sc.redo_units(this[0].side["ws"], fr.n, fr.h, fr.w, _native.splat_tile_geometry()[2])
        st = this[0].side["stats"]
        assert st[0] == 0 and st[2] == 0, st
        allowed = np.zeros((fr.n, fr.h, fr.w), bool)
        for b, ty, tx, b0, b1, marked in units:
            if marked:
                allowed[b, ty * sc.TH + b0: ty * sc.TH + b1, tx * sc.TW: (tx + 1) * sc.TW] = True
        ref = _oracle_splat(inp, **kw)
        v, den, warped = _np(res[0]), _np(res[2]), _np(res[3])
        rv, rden = _np(ref[0]), _np(ref[2])
        diff = (v.view(np.uint32) != rv.view(np.uint32)).any(1) | (den.view(np.uint32) != rden.view(np.uint32)) | (warped != _np(ref[3]))
        if holes:
            m, rm = _np(res[1]), _np(ref[1])
            diff |= m.view(np.uint32) != rm.view(np.uint32)
            np.testing.assert_allclose(m, rm, rtol=2e-5, atol=2e-5)
            assert np.array_equal(m == 1, rm == 1)
        assert not (diff & ~allowed).any(), "%d pixels outside the folded bands differ from the oracle" % int((diff & ~allowed).sum())
        _finite_where_ref(v, rv, "values")
        np.testing.assert_allclose(v, rv, rtol=2e-5, atol=2e-5 * float(np.abs(rv).max()))
        np.testing.assert_allclose(den, rden, rtol=2e-5, atol=2e-5 * float(rden.max()))
        assert np.array_equal(warped, _np(ref[3]))

    case("splat.fold-c%d-holes%d" % (c, holes), "_splat_fwd_raw", functools.partial(_cells_inputs, "fold", c, holes), run,
         callees=("_fallback_accum",), atomic=atomic, options=functools.partial(_splat_stats, 2))
    this.append(CASES[-1])


_add_fold(3, True)
_add_fold(2, False)


def _shrink(h, w, k, cx, cy):
    xs = torch.arange(w, dtype=torch.float32).view(1, 1, 1, w)
    ys = torch.arange(h, dtype=torch.float32).view(1, 1, h, 1)
    return torch.cat([(-k * (xs - cx)).expand(1, 1, h, w), (-k * (ys - cy)).expand(1, 1, h, w)], 1).contiguous()


FULL_KW = dict(want_valid=True, want_density=True, want_warped=True)


def _queue_inputs():
    """tests/test_gpu_parity.py::test_queue_capacity_exceeded_takes_the_two_pass_path"""
    n, c, h, w = 1, 2, 256, 384
    g = torch.Generator().manual_seed(8)
    data = torch.rand(n, c, h, w, generator=g) * 10
    wm = torch.rand(n, h, w, generator=g) > 0.1
    return dict(flow=_shrink(h, w, 0.8, 190.3, 120.7), data=data, wm=wm, ca=wm.clone())


def _run_full(nat, ofl, g):
    return nat.splat_fwd(g["flow"], g["data"], **dict(FULL_KW, **_splat_kw(g)))


case("splat.queue_capacity", "_splat_fwd_raw", _queue_inputs, _run_full, callees=("_fallback_accum",),
     atomic=_bars_splat(FULL_KW, 3e-5, 3e-4, 1e-4))


def _list_limit_inputs():
    """tests/test_gpu_parity.py::test_a_fold_beyond_the_list_limit_falls_back_per_tile"""
    n, c, h, w = 1, 2, 128, 96
    ys = torch.arange(h, dtype=torch.float32).view(1, 1, h, 1)
    v = torch.where((ys >= 32) & (ys < 112), 60.4 - ys, torch.zeros_like(ys)).expand(n, 1, h, w)
    g = torch.Generator().manual_seed(4)
    return dict(flow=torch.cat([torch.full((n, 1, h, w), 0.3), v], 1).contiguous(), data=torch.rand(n, c, h, w, generator=g) * 10)


LIST_KW = dict(want_density=True, want_warped=True, occlude=False)
case("splat.list_limit", "_splat_fwd_raw", _list_limit_inputs,
     lambda nat, ofl, g: nat.splat_fwd(g["flow"], g["data"], **LIST_KW), callees=("_fallback_accum",),
     atomic=_bars_splat(LIST_KW, 2e-5, 2e-4, 1e-5))


def _slots_inputs():
    """tests/test_gpu_parity.py::test_fallback_accumulator_is_bounded_and_served_in_rounds: images 0, 2, 4 fall back, 1 and 3 do not"""
    n, c, h, w = 5, 2, 256, 384
    shrink = _shrink(h, w, 0.9, 190.3, 120.7)
    smooth = _smooth(2, h, w, 3.0, 31)
    g = torch.Generator().manual_seed(18)
    data = torch.rand(n, c, h, w, generator=g) * 10
    wm = torch.rand(n, h, w, generator=g) > 0.1
    return dict(flow=torch.cat([shrink, smooth[:1], shrink * 0.97, smooth[1:], shrink * 1.02], 0).contiguous(), data=data, wm=wm, ca=wm.clone())


for _slots in (1, 2):
    case("splat.fallback_slots-%d" % _slots, "_fallback_accum", _slots_inputs, _run_full, callees=("_splat_fwd_raw",),
         atomic=_bars_splat(FULL_KW, 3e-5, 3e-4, 1e-4, exact_images=(1, 3)),
         options=functools.partial(_option, "set_splat_fallback_slots", _slots))


def _passes_inputs(rough):
    """Three images, one per pass (tests/test_gpu_parity.py::test_only_the_flagged_image_leaves_the_exact_path); rough: image 0's
    lists overflow, so that pass takes the two-pass path and the later passes find the workspace as it left it."""
    n, c, h, w = 3, 2, 160, 320
    flow = _smooth(n, h, w, 1.5, 78)
    if rough:
        flow[0] += _shrink(h, w, 0.9, 150.3, 70.7)[0]
    g = torch.Generator().manual_seed(13)
    return dict(flow=flow, data=torch.rand(n, c, h, w, generator=g) * 100 - 20, wm=torch.rand(n, h, w, generator=g) > 0.15)


PASS_KW = dict(want_density=True, want_warped=True)
_run_pass = lambda nat, ofl, g: nat.splat_fwd(g["flow"], g["data"], **dict(PASS_KW, **_splat_kw(g)))
case("splat.passes-smooth", "_splat_fwd_raw", functools.partial(_passes_inputs, False), _run_pass, callees=("_fallback_accum",),
     control=_exact_splat_control(PASS_KW), options=functools.partial(_option, "set_splat_pass_images", 1))
case("splat.passes_rough", "_splat_fwd_raw", functools.partial(_passes_inputs, True), _run_pass, callees=("_fallback_accum",),
     atomic=_bars_splat(PASS_KW, 3e-5, 3e-5 * 120.0, 1e-5, exact_images=(1, 2)), options=functools.partial(_option, "set_splat_pass_images", 1))


def _tiled_inputs(shape, sigma, seed=21):
    """tests/test_gpu_parity.py::test_tiled_splat_matches_two_pass_and_oracle / test_exact_splat_is_bit_identical_to_the_oracle"""
    n, c, h, w = shape
    flow = _smooth(n, h, w, sigma, seed)
    flow[0, :, h // 4: h // 2, w // 4: w // 2] = 0
    g = torch.Generator().manual_seed(9)
    return dict(flow=flow, data=torch.rand(n, c, h, w, generator=g) * 100 - 20, wm=torch.rand(n, h, w, generator=g) > 0.15,
                ca=torch.rand(n, h, w, generator=g) > 0.15)


TILED_BAR = dict(rtol=3e-5, atol_v=3e-5 * 120.0, atol_den=1e-5, atol_m=3e-5)
NARROW_KW = dict(want_valid=True, want_density=True, want_warped=True)
case("splat.narrow-2x3x9x3", "_splat_fwd_raw", functools.partial(_tiled_inputs, (2, 3, 9, 3), 3.0),
     lambda nat, ofl, g: nat.splat_fwd(g["flow"], g["data"], **dict(NARROW_KW, **_splat_kw(g))),
     atomic=_bars_splat(NARROW_KW, **TILED_BAR))


@contextlib.contextmanager
def _two_pass():
    from oflibpytorch_amd import _native
    _native.set_splat_path(1)
    try:
        yield
    finally:
        _native.set_splat_path(0)


MCH_KW = dict(flow_sign=-1.0, data_sign=-1.0, want_mask_chan=True, want_density=True)
case("splat.two_pass-2x3x45x97", "_splat_fwd_raw", functools.partial(_tiled_inputs, (2, 3, 45, 97), 3.0),
     lambda nat, ofl, g: nat.splat_fwd(g["flow"], g["data"], **dict(MCH_KW, **_splat_kw(g))),
     atomic=_bars_splat(MCH_KW, **TILED_BAR), options=_two_pass)

# the in-order gather path with every by-product: density, warped mask, valid / mask channel, output flag words (bit for bit the oracle's)
for _name, _shape, _kw in [("valid", (2, 3, 37, 50), dict(want_valid=True, want_density=True, want_warped=True)),
                           ("mask_chan", (2, 3, 37, 50), dict(flow_sign=-1.0, data_sign=-1.0, want_mask_chan=True, want_density=True)),
                           ("plain", (2, 4, 40, 64), dict(want_density=True)),
                           ("round", (1, 7, 33, 45), dict(occlude=False, want_warped=True))]:
    case("splat.exact-%s-%dx%dx%dx%d" % ((_name,) + _shape), "_splat_fwd_raw", functools.partial(_tiled_inputs, _shape, 1.5, 33),
         (lambda kw: lambda nat, ofl, g: nat.splat_fwd(g["flow"], g["data"], **dict(kw, **_splat_kw(g))))(_kw),
         callees=("_fallback_accum",), control=_exact_splat_control(_kw))


def _dst_flags_control(res0, inp):
    from oracle import oracle
    ref = _oracle_splat(inp, want_valid=True, want_dst_flags=True)
    for k in (0, 1, 4):
        _eq_values(_np(res0[k]), _np(ref[k]), "splat result %d" % k)
    assert _np(res0[4]).tolist() == [int(x) for x in oracle.flow_flags(_np(res0[0]), _np(res0[1]))]


case("splat.dst_flags-3x2x70x132", "_splat_fwd_raw", functools.partial(_tiled_inputs, (3, 2, 70, 132), 1.5, 33),
     lambda nat, ofl, g: nat.splat_fwd(g["flow"], g["data"], want_valid=True, want_dst_flags=True, **_splat_kw(g)),
     callees=("_fallback_accum",), control=_dst_flags_control)


def _data_b_inputs():
    inp = _tiled_inputs((2, 2, 37, 50), 1.5, 33)
    g = torch.Generator().manual_seed(19)
    inp["data_b"] = torch.rand(2, 2, 37, 50, generator=g) * 30
    return inp


case("splat.data_b-2x2x37x50", "_splat_fwd_raw", _data_b_inputs,
     lambda nat, ofl, g: nat.splat_fwd(g["flow"], g["data"], want_valid=True, **_splat_kw(g)),
     callees=("_fallback_accum",), control=_exact_splat_control(dict(want_valid=True)))


def _xy_inputs():
    """tests/test_gpu_parity.py::test_tiled_splat_explicit_positions"""
    g = torch.Generator().manual_seed(4)
    n, c, h, w = 2, 3, 40, 64
    x = torch.rand(n, h, w, generator=g) * (w + 6) - 3
    y = torch.rand(n, h, w, generator=g) * (h + 6) - 3
    return dict(xs=x, ys=y, data=torch.rand(n, c, h, w, generator=g) * 50, wm=torch.rand(n, h, w, generator=g) > 0.2)


def _xy_control(res0, inp):
    from oracle import oracle
    ref, rden = oracle.grid_from_unstructured_data(_np(inp["xs"]), _np(inp["ys"]), _np(inp["data"]), _np(inp["wm"]))
    np.testing.assert_allclose(_np(res0[0]), ref, rtol=3e-5, atol=3e-3)
    np.testing.assert_allclose(_np(res0[2]), rden, rtol=3e-5, atol=1e-5)


case("splat.xy-2x3x40x64", "_splat_fwd_raw", _xy_inputs,
     lambda nat, ofl, g: nat.splat_fwd(None, g["data"], occlude=False, want_density=True, **_splat_kw(g)),
     callees=("_fallback_accum",), control=_xy_control)


def _add_splat_win(shape, pad):
    n, c, hp, wp = shape
    h, w = hp - pad[0] - pad[1], wp - pad[2] - pad[3]

    def build():
        g = torch.Generator().manual_seed(21)
        f = _smooth(n, h, w, 1.5, 5)
        f[0, :, : h // 4] = 0
        return dict(flow=f, wm=torch.rand(n, h, w, generator=g) > 0.15, data=torch.rand(n, c, hp, wp, generator=g) * 200,
                    ca=torch.rand(n, hp, wp, generator=g) > 0.1)

    def run(nat, ofl, g):
        res = nat.splat_fwd_win(g["flow"], g["data"], (pad[0], pad[2]), weight_mask=g["wm"], chan_mask_a=g["ca"], want_valid=True)
        assert res is not None
        return res

    def control(res0, inp):
        import oracle_backend as ob
        ref = ob.splat_fwd_win(inp["flow"], inp["data"], (pad[0], pad[2]), weight_mask=inp["wm"], chan_mask_a=inp["ca"], want_valid=True)
        assert np.array_equal(_np(res0[1]), _np(ref[1]))
        np.testing.assert_allclose(_np(res0[0]), _np(ref[0]), rtol=3e-5, atol=3e-3)

    case("splat.win-%dx%dx%dx%d" % shape, "splat_fwd_win", build, run, callees=("_fallback_accum",), control=control)


for _shape, _pad in PADS[:3]:
    _add_splat_win(_shape, _pad)


def _sum_inputs(shape):
    """tests/test_gpu_parity.py::test_splat_sum_is_the_unnormalised_splat_bit_for_bit"""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(c + h)
    return dict(flow=_smooth(n, h, w, 1.5, 91), data=torch.rand(n, c, h, w, generator=g) * 10 - 3)


def _sum_control(res0, inp):
    from test_gpu_parity import _splat_sum_reference
    _eq_values(_np(res0), _splat_sum_reference(_np(inp["flow"]), _np(inp["data"]), -1.0, -1.0), "splat_sum")


for _shape in [(2, 3, 40, 56), (1, 5, 33, 45)]:
    case("splat.sum-%dx%dx%dx%d" % _shape, "splat_sum", functools.partial(_sum_inputs, _shape),
         lambda nat, ofl, g: nat.splat_sum(g["flow"], g["data"], flow_sign=-1.0, data_sign=-1.0), callees=("_fallback_accum",),
         control=_sum_control)


def _add_half_splat(kind, valid, out_half):
    """tests/test_gpu_splat_cells.py::test_fp16_flow_and_data_are_bit_exact"""
    def run(nat, ofl, g):
        kw = dict(weight_mask=g["wm"], want_valid=valid, out_half=out_half)
        if valid:
            kw["chan_mask_a"] = g["ca"]
        res = nat.splat_fwd(g["flow"], g["data"], **kw)
        assert "DF16_" in nat.last_kernel_name(demangle=False)
        return res[:2]

    def control(res0, inp):
        import oracle_backend as ob
        ref = ob.splat_fwd(inp["flow"].float(), inp["data"].float(), weight_mask=inp["wm"], chan_mask_a=inp["ca"], want_valid=valid)
        want = _np(ref[0]).astype(np.float16) if out_half else _np(ref[0])
        _eq_values(_np(res0[0]), want, "values")
        if valid:
            assert np.array_equal(_np(res0[1]), _np(ref[1]))

    case("splat.half-%s-valid%d-half%d" % (kind, valid, out_half), "_splat_fwd_half", functools.partial(_cells_inputs, kind, 2, valid, True),
         run, callees=("_fallback_accum",), control=control)


_add_half_splat("first", True, False)
_add_half_splat("second", False, True)


# ==================================================================================================================================
# gradients (tests/grad_cases64.py, tests/grad_oracle64.py)
# ==================================================================================================================================
GRAD_FAMILIES = ("smooth", "zero_disc")


def _excess(got, ref, key, what):
    import grad_oracle64 as go
    g = _np(got.float())
    _finite_where_ref(g, ref[0], what)                          # (ref: value, magnitude sum, term count)
    ex = go.excess(g, ref, go.R[key])
    print("%-60s %-16s err/bound %.4g" % (what, key, ex))
    assert ex <= 1.0, "%s %s: |got - ref64| reaches %.4g of the per-element bound" % (what, key, ex)


def _sid(shape):
    return "x".join(str(s) for s in shape)


def _add_warp_grad(shape, family):
    n, h, w = shape
    c = 3

    def build():
        return dict(flow=gc.flow(family, n, h, w), src=gc.image(n, c, h, w), gout=gc.upstream(n, c, h, w))

    def run(nat, ofl, g):
        return nat.warp_bwd_grad(g["flow"], g["src"], g["gout"], flow_sign=-1.0, g_scale=gc.G_SCALE)

    def ref_of(inp):
        import grad_oracle64 as go
        return go.warp_grad(_np(inp["flow"]), _np(inp["src"]), _np(inp["gout"]), -1.0, gc.G_SCALE)

    def control(res0, inp):
        ref = ref_of(inp)
        _excess(res0[0], ref['grad_src'], 'warp.grad_src', "warp_bwd_grad %s %s" % (family, shape))
        _excess(res0[1], ref['grad_flow'], 'warp.grad_flow', "warp_bwd_grad %s %s" % (family, shape))

    def atomic(res, inp, res0):                               # (W < 4: grad_src by float atomics; grad_flow stays bit for bit)
        control(res, inp)
        dm.assert_same_bits(res[1], res0[1], "grad_flow")

    case("grad.warp-%s-%s" % (_sid(shape), family), "warp_bwd_grad", build, run, callees=() if w < 4 else ("splat_sum", "_fallback_accum"),
         control=None if w < 4 else control, atomic=atomic if w < 4 else None)


def _add_warp_grad_x16(shape, family, dtype):
    n, h, w = shape
    c = 3

    def build():
        return dict(flow=gc.flow(family, n, h, w), src=gc.image(n, c, h, w).to(dtype), gout=gc.upstream(n, c, h, w).to(dtype))

    def prepare(nat, ofl, g):                                 # the fp32 route on the widened tensors, rounded once
        gs, _ = nat.warp_bwd_grad(g["flow"], g["src"].float(), g["gout"].float(), flow_sign=1.0, g_scale=-1.0, want_flow=False)
        return {"ref_src": gs.to(dtype)}

    def run(nat, ofl, g):
        res = nat.warp_bwd_grad_x16(g["flow"], g["src"], g["gout"], flow_sign=1.0, g_scale=-1.0)     # (a source gradient: +-1 only)
        assert res is not None
        this[0].side["ref_src"] = g["ref_src"]
        return res

    def control(res0, inp):
        import grad_oracle64 as go
        ref = go.warp_grad(_np(inp["flow"]), _np(inp["src"].float()), _np(inp["gout"].float()), 1.0, -1.0)
        _excess(res0[1], ref['grad_flow'], 'warp.grad_flow', "warp_bwd_grad_x16 %s %s %s" % (family, shape, dtype))
        assert res0[0].dtype == dtype
        assert torch.equal(res0[0].view(torch.int16), this[0].side["ref_src"].view(torch.int16)), "grad_src differs from the fp32 route's"

    this = []
    case("grad.warp_x16-%s-%s-%s" % (_sid(shape), family, str(dtype).split(".")[1]), "warp_bwd_grad_x16", build, run,
         callees=("_splat_sum_x16", "_fallback_accum"), control=control, prepare=prepare)
    this.append(CASES[-1])


def _add_warp_grad_nhwc(shape, family):
    n, h, w = shape
    c = 4
    want_src = w >= 4

    def build():
        return dict(flow=gc.flow(family, n, h, w), src=gc.image(n, c, h, w).contiguous(memory_format=CL),
                    gout=gc.upstream(n, c, h, w).contiguous(memory_format=CL))

    def run(nat, ofl, g):
        res = nat.warp_bwd_grad_nhwc(g["flow"], g["src"], g["gout"], flow_sign=1.0, g_scale=-1.0, want_src=want_src)
        assert res is not None
        assert res[0] is None or res[0].is_contiguous(memory_format=CL)
        return res

    def control(res0, inp):
        import grad_oracle64 as go
        ref = go.warp_grad(_np(inp["flow"]), _np(inp["src"]), _np(inp["gout"]), 1.0, -1.0)
        _excess(res0[1], ref['grad_flow'], 'warp.grad_flow', "warp_bwd_grad_nhwc %s %s" % (family, shape))
        if want_src:
            _excess(res0[0], ref['grad_src'], 'warp.grad_src', "warp_bwd_grad_nhwc %s %s" % (family, shape))

    case("grad.warp_nhwc-%s-%s" % (_sid(shape), family), "warp_bwd_grad_nhwc", build, run,
         callees=("splat_sum", "_fallback_accum") if want_src else (), control=control)


def _add_splat_grad(shape, family, c):
    n, h, w = shape

    def build():
        return dict(flow=gc.flow(family, n, h, w), data=gc.image(n, c, h, w), gout=(gc.upstream(n, c, h, w) * gc.G_SCALE).contiguous(),
                    gden=gc.upstream(n, 1, h, w, 1)[:, 0].contiguous(), wm=gc.holes(n, h, w))

    def prepare(nat, ofl, g):                                 # ONE forward for all fills (on the W < 4 frame it adds with atomics)
        out, _, den, _ = nat.splat_fwd(g["flow"], g["data"], want_density=True, weight_mask=g["wm"])
        return {"out": out, "den": den}

    def run(nat, ofl, g):
        this[0].side["out"], this[0].side["den"] = g["out"], g["den"]
        return nat.splat_grad(g["flow"], g["data"], g["out"], g["den"], g["gout"], weight_mask=g["wm"], grad_density=g["gden"])

    def control(res0, inp):
        import grad_oracle64 as go
        s = this[0].side
        ref = go.splat_grad(_np(inp["flow"]), _np(inp["data"]), _np(s["out"]), _np(s["den"]), _np(inp["gout"]), _np(inp["gden"]),
                            _np(inp["wm"]), True, 1.0, None, None)
        _excess(res0[0], ref['grad_data'], 'splat.grad_data', "splat_grad %s %s C=%d" % (family, shape, c))
        _excess(res0[1], ref['grad_xy'], 'splat.grad_xy', "splat_grad %s %s C=%d" % (family, shape, c))

    this = []
    case("grad.splat-%s-%s-c%d" % (_sid(shape), family, c), "splat_grad", build, run, control=control, prepare=prepare)
    this.append(CASES[-1])


def _add_pts_grad(shape, family):
    n, h, w = shape

    def build():
        g = torch.Generator().manual_seed(6000)
        gout = (torch.randn(n, 257, 2, generator=g) * torch.logspace(-4, 0, 257).view(1, 257, 1)).contiguous()
        return dict(flow=gc.flow(family, n, h, w), pts=gc.points(n, h, w), gout=gout)

    def run(nat, ofl, g):
        return nat.sample_pts_grad(g["flow"], g["pts"], g["gout"])

    def atomic(res, inp, res0):
        import grad_oracle64 as go
        ref = go.sample_pts_grad(_np(inp["flow"]), _np(inp["pts"]), _np(inp["gout"]))
        _excess(res[0], ref['grad_flow'], 'pts.grad_flow', "sample_pts_grad %s %s" % (family, shape))
        _excess(res[1], ref['grad_pts'], 'pts.grad_pts', "sample_pts_grad %s %s" % (family, shape))
        dm.assert_same_bits(res[1], res0[1], "grad_pts")      # (no atomic writes it)

    case("grad.pts-%s-%s" % (_sid(shape), family), "sample_pts_grad", build, run, atomic=atomic)


for _shape in gc.SHAPES:
    for _family in GRAD_FAMILIES:
        _add_warp_grad(_shape, _family)
        _add_warp_grad_nhwc(_shape, _family)
        _add_pts_grad(_shape, _family)
        for _c in (1, 3, 5):
            _add_splat_grad(_shape, _family, _c)
        if _shape[2] >= 4:
            _add_warp_grad_x16(_shape, _family, torch.float16 if _family == "smooth" else torch.bfloat16)


def _epe_inputs(n, h, w):
    import test_gpu_flow_error as fe
    est, gt, em, gm = (torch.from_numpy(a.copy()) for a in fe._case(n, h, w))
    up, _ = fe._grad_case(n, h, w)
    scale = torch.from_numpy((up.astype(np.float64) / fe._oracle(n, h, w)['count']).astype(np.float32))
    return dict(est=est, gt=gt, em=em, gm=gm, scale=scale)


def _add_epe_grad(n, h, w):
    def run(nat, ofl, g):
        return nat.flow_epe_grad(g["est"], g["gt"], g["em"], g["gm"], g["scale"], want_est=True, want_gt=True)

    def control(res0, inp):
        import test_gpu_flow_error as fe
        _, want = fe._grad_case(n, h, w)
        fe._ulp_check(_np(res0[0]), want)
        fe._ulp_check(_np(res0[1]), -want)

    case("grad.epe-%dx%dx%d" % (n, h, w), "flow_epe_grad", functools.partial(_epe_inputs, n, h, w), run, control=control)


for _n, _h, _w in [(3, 5, 7), (3, 37, 53)]:
    _add_epe_grad(_n, _h, _w)


# ==================================================================================================================================
# side kernels
# ==================================================================================================================================
def _flags_inputs(n, h, w, half=False):
    g = torch.Generator().manual_seed(n * h + w)
    f = _smooth(n, h, w, 3.0, 7)
    f[0] = 0.0                                                # an image whose word stays 0
    if n > 1:
        f[1] = 5e-4                                           # non-zero, below the threshold
    m = torch.rand(n, h, w, generator=g) > 0.3
    return dict(flow=f.half() if half else f, mask=m)


def _flags_control(res0, inp):
    from oracle import oracle
    assert _np(res0).tolist() == [int(x) for x in oracle.flow_flags(_np(inp["flow"].float()), _np(inp["mask"]))]


for _shape, _half in [((3, 33, 47), False), ((2, 9, 3), False), ((3, 70, 132), True)]:
    case("side.flow_flags-%s-half%d" % (_sid(_shape), _half), "flow_flags", functools.partial(_flags_inputs, *_shape, half=_half),
         lambda nat, ofl, g: nat.flow_flags(g["flow"], g["mask"]), control=_flags_control)


def _host_flags_run(nat, ofl, g):
    keep = dict(nat._host_slots)
    nat._host_slots.clear()                                   # the slot (its device work words) is made anew, through the harness
    try:
        words = nat.flow_flags_host(g["flow"], g["mask"])
        assert words is not None
        torch.cuda.synchronize()
        return torch.tensor(words, dtype=torch.int32)
    finally:
        nat._host_slots.clear()
        nat._host_slots.update(keep)


case("side.flow_flags_host-3x33x47", "_new_host_slot", functools.partial(_flags_inputs, 3, 33, 47), _host_flags_run, control=_flags_control)


def _from_half_control(res0, inp):
    _eq_bits(_np(res0[0]), _np(inp["flow"].float()), "fp32 copy")
    _flags_control(res0[1], inp)


for _shape in [(3, 70, 132), (2, 37, 50), (1, 9, 3)]:
    case("side.flow_from_half-%s" % _sid(_shape), "flow_from_half", functools.partial(_flags_inputs, *_shape, half=True),
         lambda nat, ofl, g: nat.flow_from_half(g["flow"], g["mask"]), control=_from_half_control)


def _extents_inputs():
    n, h, w = 3, 37, 131
    g = torch.Generator().manual_seed(82)
    m = torch.rand(n, h, w, generator=g) > 0.3
    m[1] = False                                              # an image without a valid pixel next to valid ones
    return dict(flow=_smooth(n, h, w, 3.0, 81), mask=m)


def _extents_control(res0, inp):
    from oracle import oracle
    got = _np(res0)
    keep = [0, 2]
    exp = oracle.flow_extents(_np(inp["flow"])[keep], _np(inp["mask"])[keep], 1.0)
    same = (got[keep] == exp) & ((np.signbit(got[keep]) == np.signbit(exp)) | (got[keep] == 0))
    assert same.all(), (got[keep], exp)
    assert got[1, 4] == 0.0 and got[0, 4] == 1.0


case("side.flow_extents-3x37x131", "flow_extents", _extents_inputs, lambda nat, ofl, g: nat.flow_extents(g["flow"], g["mask"], 1.0),
     control=_extents_control)


def _valid_control(res0, inp):
    import oracle_backend as ob
    assert np.array_equal(_np(res0), _np(ob.warp_valid(inp["flow"], inp["mask"], -1.0, 0.9999)))


for _shape in [(2, 37, 53), (1, 64, 128)]:
    case("side.warp_valid-%s" % _sid(_shape), "warp_valid", functools.partial(_flags_inputs, *_shape),
         lambda nat, ofl, g: nat.warp_valid(g["flow"], g["mask"], -1.0, 0.9999), control=_valid_control)


def _matrix_inputs():
    from oflibpytorch_amd.utils import matrix_from_transforms
    return dict(m=torch.stack([matrix_from_transforms([['translation', -3, 4.5], ['rotation', 20, 10, 33]]),
                               matrix_from_transforms([['scaling', 15, 12, 1.25]]), torch.eye(3)]))


def _matrix_control(res0, inp):
    from oracle import oracle
    _eq_values(_np(res0), oracle.flow_from_matrix(_np(inp["m"]), 3, 37, 53, -1.0), "flow_from_matrix")


case("side.flow_from_matrix-3x37x53", "flow_from_matrix", _matrix_inputs, lambda nat, ofl, g: nat.flow_from_matrix(g["m"], 3, 37, 53, -1.0),
     control=_matrix_control)


def _words_inputs(n):
    g = torch.Generator().manual_seed(3)
    return dict(words=torch.randint(0, 32, (n,), generator=g, dtype=torch.int32) & 0b10110)


def _words_control(res0, inp):
    words, expect = inp["words"].tolist(), 0
    for v in words:
        expect |= v
    out = _np(res0).tolist()
    assert out[:len(words)] == words and out[len(words):] == [(expect >> k) & 1 for k in range(5)]


for _n in (1, 65, 300):
    case("side.flag_words_or-%d" % _n, "flag_words_or", functools.partial(_words_inputs, _n),
         lambda nat, ofl, g: nat.flag_words_or(g["words"]), control=_words_control)


def _pts_inputs(m):
    n, h, w = 2, 37, 70
    pts = gc.points(n, h, w) if m else torch.zeros(n, 0, 2)
    return dict(flow=gc.flow("smooth", n, h, w), pts=pts)


def _pts_control(res0, inp):
    from oracle import oracle
    assert tuple(res0.shape) == tuple(inp["pts"].shape)
    if inp["pts"].shape[1]:
        _eq_values(_np(res0), oracle.sample_pts(_np(inp["flow"]), _np(inp["pts"])), "sample_pts")


for _m in (0, 257):
    case("side.sample_pts-m%d" % _m, "sample_pts", functools.partial(_pts_inputs, _m), lambda nat, ofl, g: nat.sample_pts(g["flow"], g["pts"]),
         control=_pts_control)


def _layout_inputs(shape, dtype, to_planes):
    g = torch.Generator().manual_seed(5)
    t = (torch.randn(*shape, generator=g) * 3).to(dtype)
    return dict(t=t.contiguous(memory_format=CL) if to_planes else t)


def _raw(t):
    """NumPy view of a tensor's elements (16-bit floats as int16: NumPy has no bfloat16)."""
    t = t.contiguous()
    return _np(t.view(torch.int16) if t.element_size() == 2 else t)


def _planes_control(res0, inp):
    assert res0.is_contiguous()
    _eq_bits(_raw(res0), _raw(inp["t"]), "planes")


def _nhwc_control(res0, inp):
    assert res0.is_contiguous(memory_format=CL) and not res0.is_contiguous()
    _eq_bits(_raw(res0), _raw(inp["t"]), "channels_last")


for _shape, _dtype in [((2, 4, 37, 53), torch.float32), ((3, 8, 33, 47), torch.bfloat16)]:
    _tag = "%s-%s" % (_sid(_shape), str(_dtype).split(".")[1])
    case("side.nhwc_to_planes-" + _tag, "_transpose", functools.partial(_layout_inputs, _shape, _dtype, True),
         lambda nat, ofl, g: nat.nhwc_to_planes(g["t"]), control=_planes_control)
    case("side.planes_to_nhwc-" + _tag, "_transpose", functools.partial(_layout_inputs, _shape, _dtype, False),
         lambda nat, ofl, g: nat.planes_to_nhwc(g["t"]), control=_nhwc_control)


def _resize_inputs():
    g = torch.Generator().manual_seed(12)
    return dict(x=torch.randn(3, 2, 37, 53, generator=g) * 4)


def _add_resize(scale):
    def control(res0, inp):
        from oracle import oracle
        _eq_values(_np(res0), oracle.resize_bilinear(_np(inp["x"]), list(scale)), "resize")

    case("side.resize-%gx%g" % scale, "resize_bilinear", _resize_inputs, lambda nat, ofl, g: nat.resize_bilinear(g["x"], scale), control=control)


for _scale in [(0.5, 0.5), (1.5, 1.5), (0.3, 2.7), (1.0, 1.0)]:
    _add_resize(_scale)


# ==================================================================================================================================
# newer families: visualise, matrix, metrics, arrows, mesh, loaders
# ==================================================================================================================================
def _vis_inputs(half=False):
    import test_gpu_visualise as tv
    n, h, w = 3, 37, 53
    flow, mask = tv._smooth(n, h, w, 5.0, 3 + h, 'cpu'), tv._mask(n, h, w, 4 + w, 'cpu')
    mask[:, 0, 0] = True
    return dict(flow=flow.half() if half else flow, mask=mask)


def _add_vis(show_mask, borders, half=False):
    def run(nat, ofl, g):
        rng, counts = nat.visualise_range(g["flow"], g["mask"])
        outs = [rng, counts]
        for mode in ('hsv', 'rgb', 'bgr'):
            for layout in (nat.VIS_PLANES, nat.VIS_INTERLEAVED):
                outs.append(nat.visualise(g["flow"], rng, mode, g["mask"], show_mask, borders, layout))
        return tuple(outs)

    def control(res0, inp):
        import vis_oracle as vo
        v, m = _np(inp["flow"].float()), _np(inp["mask"])
        mag, _ = vo.cart_to_polar(vo.threshold(v[:, 0]), vo.threshold(v[:, 1]))
        rng = vo.default_range(mag, m)
        assert np.array_equal(_np(res0[0]), rng)
        hsv = vo.hsv_planes(v, m, show_mask, borders, rng)
        rgb = vo.hsv_to_rgb(hsv)
        exp = {'hsv': np.round(hsv).astype(np.uint8), 'rgb': rgb, 'bgr': rgb[..., ::-1]}
        for k, mode in enumerate(('hsv', 'rgb', 'bgr')):
            assert np.array_equal(_np(res0[2 + 2 * k]), np.moveaxis(exp[mode], -1, 1)), mode
            assert np.array_equal(_np(res0[3 + 2 * k]), exp[mode]), mode

    case("new.visualise-mask%d-borders%d-half%d" % (show_mask, borders, half), "visualise", functools.partial(_vis_inputs, half), run,
         callees=("visualise_range",), control=control)


for _sm, _b in [(False, False), (True, False), (False, True), (True, True)]:
    _add_vis(_sm, _b)
_add_vis(True, True, half=True)


def _fit_inputs(ref):
    """An outlier flow of a known matrix (tests/test_gpu_matrix.py::_inputs, made by the oracle's generator instead of the device's)
    beside an image with one valid pixel: too few points for any fit."""
    from oracle import oracle
    from oflibpytorch_amd.utils import matrix_from_transforms
    h, w = 40, 56
    rs = np.random.RandomState(5)
    mat = matrix_from_transforms([['translation', 2, 1], ['rotation', w / 5, h / 5, 30], ['scaling', w / 20, h / 10, 1.1]])
    if ref == 't':
        mat = torch.linalg.inv(mat.double()).float()
    vecs = oracle.flow_from_matrix(mat.numpy()[None], 1, h, w, 1.0 if ref == 's' else -1.0).astype(np.float32)
    bad = rs.rand(1, 1, h, w) < 0.3
    vecs = np.where(bad, ((rs.rand(1, 2, h, w) - 0.5) * 200).astype(np.float32), vecs)
    vecs = np.ascontiguousarray(np.concatenate([vecs, vecs]), np.float32)
    mask = rs.rand(2, h, w) > 0.1
    mask[1] = False
    mask[1, 3, 4] = True
    return dict(flow=torch.from_numpy(vecs), mask=torch.from_numpy(mask))


def _add_fit(dof, method, ref):
    def run(nat, ofl, g):
        return nat.matrix_fit(g["flow"], ref, g["mask"], dof, method)

    def control(res0, inp):
        import matrix_oracle as mo
        from test_gpu_matrix import ORACLE_BAR
        got, info = _np(res0[0]), _np(res0[1])
        exp, einfo = mo.fit(_np(inp["flow"])[:1], ref, _np(inp["mask"])[:1], dof, method)
        assert np.array_equal(info[0], einfo[0]) and einfo[0, 3] == 0, (info.tolist(), einfo.tolist())
        assert float(np.abs(got[0] - exp[0]).max() / np.abs(exp[0]).max()) <= ORACLE_BAR
        assert info[1, 0] == 1 and info[1, 3] != 0, info.tolist()      # the failed image: its count and its status are written

    case("new.matrix_fit-dof%d-%s-%s" % (dof, method, ref), "matrix_fit", functools.partial(_fit_inputs, ref), run, control=control)


for _k, (_dof, _method) in enumerate([(4, 'ransac'), (4, 'lmeds'), (6, 'ransac'), (6, 'lmeds'), (8, 'lms'), (8, 'ransac'), (8, 'lmeds')]):
    _add_fit(_dof, _method, 'st'[_k % 2])


def _error_inputs():
    import test_gpu_flow_error as fe
    est, gt, em, gm = (torch.from_numpy(a.copy()) for a in fe._case(3, 37, 53))
    em[2] = False                                             # an image with count 0
    return dict(est=est, gt=gt, em=em, gm=gm)


def _add_error(thresholds, want_map):
    def run(nat, ofl, g):
        return nat.flow_error(g["est"], g["gt"], g["em"], g["gm"], thresholds, want_map)

    def control(res0, inp):
        import flow_error_oracle as feo
        ref = feo.score(_np(inp["est"]), _np(inp["gt"]), _np(inp["em"]), _np(inp["gm"]), thresholds)
        rec = _np(res0[0])
        assert rec.shape == (3, 16) and not rec[:, 14:].any() and not rec[:, 3 + len(thresholds):7].any()
        assert rec[:, 0].tolist() == ref['count'].tolist() and rec[2, 0] == 0
        assert rec[:, 2].tolist() == ref['max'].tolist() and rec[:, 7].tolist() == ref['n_fl'].tolist()
        assert rec[:, 8:11].tolist() == ref['speed_count'].tolist()
        if thresholds:
            assert rec[:, 3:3 + len(thresholds)].tolist() == ref['n_over'].tolist()
        for i in range(3):
            assert abs(rec[i, 1] - ref['sum'][i]) <= ref['count'][i] * 2.0 ** -52 * ref['sum'][i]
        if want_map:
            _eq_bits(_np(res0[1]), ref['map'], "epe map")

    case("new.flow_error-thr%d-map%d" % (len(thresholds), want_map), "flow_error", _error_inputs, run, control=control)


for _thr, _map in [((), False), ((), True), ((1, 3, 5, 7), False), ((1, 3, 5, 7), True)]:
    _add_error(_thr, _map)


def _arrows_inputs(half=False):
    import test_gpu_arrows as ta
    n, h, w = 3, 37, 53
    flow, mask = ta._smooth(n, h, w, 5.0, 3 + h, 'cpu'), ta._mask(n, h, w, 4 + w, 'cpu')
    bg = np.stack([ta._background(h, w, 7 + i) for i in range(n)])
    return dict(flow=flow, mask=mask, img=torch.from_numpy(bg))


def _add_arrows(ref, grid, thickness, colour, show, layout):
    def run(nat, ofl, g):
        sc = nat.arrows_scale(g["flow"], grid)
        out = nat.arrows(g["flow"], ref, grid, sc, thickness, colour, g["img"], True, g["mask"], show, show, layout)
        return sc, out

    def control(res0, inp):
        import arrows_oracle as ao
        exp, s = ao.visualise_arrows(_np(inp["flow"]), ref, _np(inp["mask"]), grid, _np(inp["img"]), None, show, show, colour, thickness,
                                     return_scaling=True)
        assert np.float32(_np(res0[0])[0]).view(np.uint32) == np.float32(s).view(np.uint32)
        got = _np(res0[1])
        assert np.array_equal(got if layout == 1 else np.moveaxis(got, 1, -1), exp)

    case("new.arrows-%s-g%d-t%d-c%d-show%d-l%d" % (ref, grid, thickness, colour is not None, show, layout), "arrows", _arrows_inputs, run,
         callees=("arrows_scale",), control=control)


_add_arrows('t', 10, 1, None, False, 0)
_add_arrows('s', 5, 2, (10, 200, 30), True, 1)
_add_arrows('t', 2, 6, None, True, 1)


def _mesh_inputs(u8):
    import test_gpu_mesh as tm
    n, c, h, w = 2, 3, 33, 47
    data = tm._data(n, c, h, w, 3)
    return dict(flow=tm._smooth(n, h, w, 3.0, 2), data=data.to(torch.uint8) if u8 else data / 255, mask=tm._holes(n, h, w, 4))


def _add_mesh(u8):
    def run(nat, ofl, g):
        return nat.mesh_apply(g["flow"], g["data"], mask=g["mask"], round_mode=nat.ROUND_U8 if u8 else nat.ROUND_NONE, want_inside=True,
                              want_owner=True)

    def control(res0, inp):
        import mesh_oracle as mo
        for b in range(2):
            want, w_inside, w_owner = mo.mesh_apply(_np(inp["flow"])[b], _np(inp["data"])[b], _np(inp["mask"])[b], 1.0,
                                                    mo.ROUND_U8 if u8 else mo.ROUND_NONE)
            assert np.array_equal(_np(res0[2])[b], w_owner) and np.array_equal(_np(res0[1])[b], w_inside)
            _eq_bits(_np(res0[0])[b], want, "mesh values, image %d" % b)

    case("new.mesh_apply-u8%d" % u8, "mesh_apply", functools.partial(_mesh_inputs, u8), run, callees=("_mesh_plan",), control=control, boolish=(1,))


_add_mesh(False)
_add_mesh(True)


def _mesh_pts_inputs(m):
    import test_gpu_mesh as tm
    h, w = 41, 77
    g = torch.Generator().manual_seed(52)
    pts = torch.rand(2, max(m, 1), 2, generator=g) * torch.tensor([h + 4.0, w + 4.0]) - 2.0
    pts[:, :40] = pts[:, :40].round()
    pts[0, min(40, max(m, 1) - 1)] = float('nan')
    return dict(flow=tm._smooth(2, h, w, 3.0, 51), pts=pts[:, :m].contiguous())


def _mesh_pts_control(res0, inp):
    import mesh_oracle as mo
    for b in range(2):
        if inp["pts"].shape[1]:
            wv, wi = mo.mesh_points(_np(inp["flow"])[b], _np(inp["pts"])[b])
            assert np.array_equal(_np(res0[1])[b], wi)
            _eq_bits(_np(res0[0])[b], wv, "mesh_points, image %d" % b)


for _m in (0, 500):
    case("new.mesh_points-m%d" % _m, "mesh_points", functools.partial(_mesh_pts_inputs, _m),
         lambda nat, ofl, g: nat.mesh_points(g["flow"], g["pts"]), callees=("_mesh_plan",) if _m else (), control=_mesh_pts_control, boolish=(1,))


def _kitti_inputs(n, h, w, kind):
    import test_gpu_loaders as tl
    s = tl._kitti_samples(n, h, w, kind, np.random.RandomState(100 * n + w))
    return dict(raw=torch.from_numpy(np.ascontiguousarray(s.astype('>u2').view(np.uint8).reshape(n, -1))), s=s)


def _add_kitti(n, h, w, kind, want_mask):
    def run(nat, ofl, g):
        return nat.decode_kitti(g["raw"], h, w, want_mask)

    def control(res0, inp):
        from oracle import oracle
        s = inp["s"]
        want = np.ascontiguousarray(np.moveaxis(((s[..., :2].astype(np.float64) - 2 ** 15) / 64).astype(np.float32), -1, 1))
        _eq_bits(_np(res0[0]), want, "vecs")
        if want_mask:
            _eq_bits(_np(res0[1].view(torch.uint8)), (s[..., 2] > 0).astype(np.uint8), "mask bytes")
        assert _np(res0[2]).tolist() == [int(x) for x in oracle.flow_flags(want, (s[..., 2] > 0) if want_mask else None)]

    case("new.decode_kitti-%dx%dx%d-%s-mask%d" % (n, h, w, kind, want_mask), "decode_kitti", functools.partial(_kitti_inputs, n, h, w, kind), run,
         control=control)


_add_kitti(3, 5, 65, 'random', True)
_add_kitti(2, 3, 23, 'last', True)
_add_kitti(3, 7, 13, 'invalid', False)


def _flo_inputs(n, h, w, vkind, gkind):
    import test_gpu_loaders as tl
    rng = np.random.RandomState(200 * n + w)
    v, g = tl._flo_values(n, h, w, vkind, rng), tl._grey(n, h, w, gkind, rng)
    return dict(raw=torch.from_numpy(v.copy()), grey=None if g is None else torch.from_numpy(g))


def _add_flo(n, h, w, vkind, gkind):
    def run(nat, ofl, g):
        return nat.decode_flo(g["raw"], g["grey"])

    def control(res0, inp):
        from oracle import oracle
        v = _np(inp["raw"])
        want = np.ascontiguousarray(np.moveaxis(v, -1, 1))
        _eq_bits(_np(res0[0]), want, "vecs")
        m = None
        if inp["grey"] is not None:
            m = _np(inp["grey"]) == 0
            _eq_bits(_np(res0[1].view(torch.uint8)), m.astype(np.uint8), "mask bytes")
        assert _np(res0[2]).tolist() == [int(x) for x in oracle.flow_flags(want, m)]

    case("new.decode_flo-%dx%dx%d-%s-%s" % (n, h, w, vkind, gkind), "decode_flo", functools.partial(_flo_inputs, n, h, w, vkind, gkind), run,
         control=control)


_add_flo(3, 5, 65, 'random', 'random')
_add_flo(2, 3, 23, 'small', 'last')
_add_flo(3, 7, 13, 'random', 'none')


# ==================================================================================================================================
# Flow-level chains: a dirty intermediate crossing primitives
# ==================================================================================================================================
def _chain_inputs():
    """tests/test_gpu_parity.py::test_fused_combine_equals_the_operator_chain, on a smaller frame"""
    n, h, w = 2, 70, 132
    g = torch.Generator().manual_seed(41)
    mk = lambda s: torch.nn.functional.interpolate(torch.randn(n, 2, 5, 6, generator=g) * s, size=(h, w), mode='bicubic', align_corners=True).contiguous()
    return dict(f1=mk(3.0), f2=mk(2.0), m1=torch.rand(n, h, w, generator=g) > 0.05, m2=torch.rand(n, h, w, generator=g) > 0.05)


def _add_combine(mode):
    def run(nat, ofl, g):
        outs = []
        for sr in 'st':
            for orf in 'st':
                res = ofl.Flow(g["f1"], sr, g["m1"]).combine(ofl.Flow(g["f2"], orf, g["m2"]), mode, 't' if sr == orf else 's')
                outs += [res.vecs, res.mask]
        return tuple(outs)

    def control(res0, inp):
        import oflibpytorch_amd as ofl
        from oflibpytorch_amd import flow_class
        dev = res0[0].device
        g = {k: v.to(dev) for k, v in inp.items()}
        flow_class._COMBINE_FUSED = False                     # the operator chain: the existing test's expectation
        try:
            ref = run(None, ofl, g)
        finally:
            flow_class._COMBINE_FUSED = True
        for k, (a, b) in enumerate(zip(res0, ref)):
            assert torch.equal(a, b), "combine mode %d: result %d differs from the operator chain" % (mode, k)

    case("chain.combine-mode%d" % mode, ("_splat_fwd_raw", "_warp_bwd_lean", "_warp_bwd_raw"), _chain_inputs, run, control=control)


for _mode in (1, 2, 3):
    _add_combine(_mode)


def _switch_run(nat, ofl, g):
    outs = []
    for ref in 'st':
        res = ofl.Flow(g["f1"], ref, g["m1"]).switch_ref()
        outs += [res.vecs, res.mask]
    return tuple(outs)


def _switch_control(res0, inp):
    from oracle import oracle
    for k, ref in enumerate('st'):
        v, m, _ = oracle.switch_ref(_np(inp["f1"]), ref, _np(inp["m1"]))
        assert np.array_equal(_np(res0[2 * k + 1]), m), ref
        np.testing.assert_allclose(_np(res0[2 * k]), v, rtol=3e-5, atol=3e-4)


case("chain.switch_ref", ("_splat_fwd_raw",), _chain_inputs, _switch_run, control=_switch_control)


def _add_padded_apply(ref):
    (n, c, hp, wp), pad = PADS[0]
    h, w = hp - pad[0] - pad[1], wp - pad[2] - pad[3]

    def build():
        g = torch.Generator().manual_seed(21)
        f = _smooth(n, h, w, 1.5, 5)
        f[0, :, : h // 4] = 0
        return dict(f=f, m=torch.rand(n, h, w, generator=g) > 0.15, img=torch.rand(n, c, hp, wp, generator=g) * 200,
                    tm=torch.rand(n, hp, wp, generator=g) > 0.1)

    def run(nat, ofl, g):
        fl = ofl.Flow(g["f"], ref, g["m"])
        outs = []
        for cut in (True, False):
            outs += list(fl.apply(g["img"], target_mask=g["tm"], return_valid_area=True, consider_mask=True, padding=pad, cut=cut))
        return tuple(outs)

    def control(res0, inp):
        import oflibpytorch_amd as ofl
        dev = res0[0].device
        g = {k: v.to(dev) for k, v in inp.items()}
        padded = ofl.Flow(g["f"], ref, g["m"]).pad(pad, mode='constant' if ref == 't' else 'replicate')
        exp = padded.apply(g["img"], target_mask=g["tm"], return_valid_area=True, consider_mask=True)
        for k, cut in enumerate((True, False)):
            e = tuple(x[..., pad[0]:pad[0] + h, pad[2]:pad[2] + w] for x in exp) if cut else exp
            assert torch.equal(res0[2 * k + 1], e[1]), (ref, cut)
            assert torch.equal(res0[2 * k], e[0]), (ref, cut)

    case("chain.apply_padding-%s" % ref, ("warp_bwd_win" if ref == 't' else "splat_fwd_win",), build, run, control=control)


for _ref in 'ts':
    _add_padded_apply(_ref)


# ==================================================================================================================================
# the test
# ==================================================================================================================================
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tier needs a HIP device"
    from oflibpytorch_amd import _native
    _native.load_library()
    return torch.device('cuda', 0)


def _to_device(v, dev):
    if isinstance(v, torch.Tensor):
        return v.to(dev)
    if isinstance(v, (tuple, list)) and v and all(isinstance(x, torch.Tensor) for x in v):
        return tuple(x.to(dev) for x in v)
    return v


def _guard(h, v, name):
    if isinstance(v, torch.Tensor):
        return h.guarded(v, name)
    if isinstance(v, tuple) and v and all(isinstance(x, torch.Tensor) for x in v):
        return tuple(h.guarded(x, "%s[%d]" % (name, i)) for i, x in enumerate(v))
    return v


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_same_bits_on_dirty_guarded_memory(case, dev):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _native
    inp = case.build()
    on_dev = {k: _to_device(v, dev) for k, v in inp.items()}
    if case.prepare is not None:
        on_dev.update(case.prepare(_native, ofl, on_dev))
    res0 = None
    for fill in dm.FILLS:
        what = "%s, fill 0x%02X" % (case.id, fill)
        h = dm.Harness(fill)
        g = {k: _guard(h, v, k) for k, v in on_dev.items()}
        try:
            with (case.options() if case.options is not None else contextlib.nullcontext()):
                with h:
                    res = case.run(_native, ofl, g)
                torch.cuda.synchronize()
        except RuntimeError as exc:
            if "illegal memory access" in str(exc) or "HIP error" in str(exc):
                pytest.exit("%s: the device faulted (%s): nothing more is launched on it" % (what, exc), returncode=3)
            raise
        # 3. no stray write, no written input
        h.check_guards()
        h.check_inputs_unchanged()
        # 4. the harness was in the path
        assert h.log, "%s: nothing was allocated through the harness" % what
        named = (case.primitive,) if isinstance(case.primitive, str) else case.primitive    # (a Flow-level chain: any of these)
        assert set(named) & set(h.callers()), "%s: %s allocated nothing (callers: %s)" % (what, named, h.callers())
        missing = set(case.callees) - set(h.callers())
        assert not missing, "%s: declared callees that allocated nothing: %s" % (what, sorted(missing))
        # 1. bool bytes; the same bits under every fill (or the bar of the exception list)
        dm.assert_bool_bytes(res, what)
        flat = dm.flatten(res)
        for k in case.boolish:
            assert not flat[k].numel() or int(dm.as_bytes(flat[k]).max()) <= 1, "%s: uint8 result %d holds a byte that is neither 0 nor 1" % (what, k)
        try:
            if fill == dm.FILLS[0]:
                res0 = res
                if case.control is not None:
                    case.control(res0, inp)                   # 2. the control is the pinned result
            if case.atomic is not None:
                case.atomic(res, inp, res0)
                for k, (a, b) in enumerate(zip(flat, dm.flatten(res0))):
                    if a is not None and not a.dtype.is_floating_point:
                        dm.assert_same_bits(a, b, "result %d (no float atomic writes it)" % k)
            elif fill != dm.FILLS[0]:
                dm.assert_same_bits(res, res0, "against the 0x00 run")
        except AssertionError as exc:
            raise AssertionError("%s: %s" % (what, exc)) from None
