"""GPU tier: images that carry NaN, +-inf, denormals, -0.0 and FLT_MAX through the backward warp and the forward splat.

Inputs and the splat's restated reference: tests/special_values.py (pinned on the CPU by tests/test_special_values_host.py, which
also asserts the conditions that keep these tests from passing vacuously).  Terms of "bit for bit" here (special_values.same_bits):
equal bits on finite elements, the sign of a zero included; NaN at the same positions; an infinity with the same sign.

Warp ('t' family): the expected result is the reference's, without deviation -- `oracle.G`, one case per distinct kernel name that
tests/golden/warp_kernel_choice.json records for the fp32 and the fp16-source entry points, plus the channel loop and an oversize box.

Splat ('s' family): the expected result is the restatement under RULE G: a source pixel that passes the weight mask
and the occlusion rule adds wgt * data at each of its corners inside the frame, zero weights included; excluded pixels and corners
outside the frame add nothing.  (a) every path gives every element the same class; (b) the in-order gather path is rule G bit for
bit; (c) paths that add with float atomics keep the bar of the other splat tests, rtol 2e-5 and atol 2e-5 * max |expected|, on the
finite expected elements, classes and masks exactly -- the maximum taken over the result of the same flow and masks on the finite
background alone (a few units), NOT over the planted FLT_MAX, 2e-5 of which (1e33) would let any finite value pass: an element
reached by FLT_MAX is so held to rtol 2e-5 of its own value; (d) a second run gives the same bits on the gather path, and the same
classes and masks on the atomics paths, whose additions come in no fixed order.
"""
import numpy as np
import pytest
import torch

import special_values as sv
import splat_cells as sc

pytestmark = pytest.mark.gpu
RTOL = 2e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tier needs a HIP device"
    from oflibpytorch_amd import _native
    _native.load_library()
    return torch.device('cuda', 0)


@pytest.fixture
def native():
    from oflibpytorch_amd import _native
    old = _native.collect_splat_stats
    _native.collect_splat_stats = 2
    yield _native
    _native.collect_splat_stats = old
    _native.set_splat_path(0)
    _native.set_splat_pass_images(0)
    _native.set_warp_path(0)


def _same(got, exp, what):
    assert sv.same_bits(got, exp).all(), "%s: %s" % (what, sv.describe(got, exp))


def _np(t):
    return None if t is None else t.cpu().numpy()


# ====================================================================================================================================
# the splat
# ====================================================================================================================================
def _check_exact(got, exp, what):
    """(b): values, mask channel (or valid mask), density, warped mask against the restatement, bit for bit."""
    for key in ("v", "m", "den", "warped"):
        if got.get(key) is not None:
            _same(got[key], exp[key], "%s, %s" % (what, key))


def _check_bars(got, exp, what):
    """(c): classes and masks exactly; the finite expected elements within rtol 2e-5, atol 2e-5 * exp["scale"][key], the largest
    magnitude of the same output over the finite background (special_values.background_scale)."""
    for key in ("v", "m", "den", "warped"):
        g, e = got.get(key), exp[key]
        if g is None:
            continue
        assert e.dtype == bool or 0.0 < exp["scale"][key] < 1e6, exp["scale"]      # (a background's magnitude, not FLT_MAX's)
        if e.dtype == bool:
            assert np.array_equal(g, e), "%s, %s" % (what, key)
            continue
        assert np.array_equal(sv.classes(g), sv.classes(e)), "%s, %s: classes differ at %s" % (
            what, key, np.argwhere(sv.classes(g) != sv.classes(e))[:6].tolist())
        fin = np.isfinite(e)
        np.testing.assert_allclose(g[fin], e[fin], rtol=RTOL, atol=RTOL * exp["scale"][key], err_msg="%s, %s" % (what, key))


def _check_same_class(a, b, what):
    """(a) / (d) on an atomics path: the class of every element and every bool output."""
    for key in ("v", "m", "den", "warped"):
        if a.get(key) is not None:
            assert np.array_equal(sv.classes(a[key]), sv.classes(b[key])), "%s, %s: classes differ at %s" % (
                what, key, np.argwhere(sv.classes(a[key]) != sv.classes(b[key]))[:6].tolist())


OPTIONS = {
    # weight mask, (chan_mask_a, chan_mask_b) | None, occlude, sign, what is asked for
    "masks-valid-density-warped": dict(masked=True, mch=(True, True), occlude=True, sign=1.0, want=dict(want_valid=True, want_density=True, want_warped=True)),
    "bare-warped": dict(masked=False, mch=None, occlude=True, sign=1.0, want=dict(want_warped=True)),
    "no-occlusion-density": dict(masked=True, mch=None, occlude=False, sign=1.0, want=dict(want_density=True)),
    "negated-mask-channel": dict(masked=True, mch=(True, False), occlude=True, sign=-1.0, want=dict(want_mask_chan=True, want_density=True)),
}


def _splat_call(native, dev, case, opt, half=False, out_half=False):
    """One _native.splat_fwd of the case under the option set -> dict(v, m, den, warped, stats)."""
    sign = np.float32(opt["sign"])
    flow = torch.from_numpy(case["flow"] * sign)
    data = torch.from_numpy(case["data"] * sign)
    if half:
        assert torch.equal(flow.half().float(), flow) and torch.equal(data.half().float().nan_to_num(7.0), data.nan_to_num(7.0))
        flow, data = flow.half(), data.half()
    kw = dict(flow_sign=float(sign), data_sign=float(sign), occlude=opt["occlude"], **opt["want"])
    if opt["masked"]:
        kw["weight_mask"] = torch.from_numpy(case["mask"]).to(dev)
    if opt["mch"] is not None:
        if opt["mch"][0]:
            kw["chan_mask_a"] = torch.from_numpy(case["ca"]).to(dev)
        if opt["mch"][1]:
            kw["chan_mask_b"] = torch.from_numpy(case["cb"]).to(dev)
    if out_half:
        kw["out_half"] = True
    native._last_splat_stats = None
    out = native.splat_fwd(flow.to(dev), data.to(dev), **kw)
    st = native._last_splat_stats
    n, _, h, w = case["data"].shape
    return dict(v=_np(out[0]), m=_np(out[1]), den=_np(out[2]), warped=_np(out[3]), stats=None if st is None else st.cpu().tolist(),
                kernel=native.last_kernel_name(demangle=False), batch=n,
                pass_images=int(native.load_library().ofl_splat_tiled_pass_images(n, h, w)))     # images per pass under the options in force


def _expected(h, w, c, half, opt):
    from oracle import oracle
    e = dict(sv.expected_splat(h, w, c, half, opt["occlude"], opt["masked"], opt["mch"]))
    e["scale"] = sv.background_scale(sv.expected_splat(h, w, c, half, opt["occlude"], opt["masked"], opt["mch"], finite_only=True))
    if opt["want"].get("want_valid"):
        e["m"] = oracle.theta(e["m"])
    return e


def _on_path(native, path, fn):
    """fn() on the gather path (0), the two-pass atomics path (1), or the gather path one image per pass (2)."""
    native.set_splat_path(1 if path == 1 else 0)
    native.set_splat_pass_images(1 if path == 2 else 0)
    try:
        return fn()
    finally:
        native.set_splat_path(0)
        native.set_splat_pass_images(0)


@pytest.mark.parametrize("opt", sorted(OPTIONS))
@pytest.mark.parametrize("h,w,c", sv.SPLAT_FRAMES)
def test_splat_follows_rule_g_on_every_path(h, w, c, opt, dev, native):
    """_native.splat_fwd on the three routes a frame can take -- the gather path, the two-pass atomics path, the gather path in several
    passes -- twice each: (a), (b), (c), (d) of the module docstring.  The flows are smooth apart from the named positions: the call's
    statistics must say that no image fell back and no tile left the exact path."""
    o = OPTIONS[opt]
    case = sv.make_splat(h, w, c)
    exp = _expected(h, w, c, False, o)
    runs = {p: [_on_path(native, p, lambda: _splat_call(native, dev, case, o)) for _ in range(2)] for p in (0, 1, 2)}
    for p in (1, 2):                                                     # (a)
        _check_same_class(runs[p][0], runs[0][0], "(a) %s against the gather path" % ("two-pass path", "gather path in passes")[p - 1])
    assert all(r["pass_images"] == 1 < r["batch"] for r in runs[2]) and runs[0][0]["pass_images"] == runs[0][0]["batch"]   # several passes / one
    for p in (0, 2):
        for r in runs[p]:
            assert r["stats"] is not None and r["stats"][0] == 0 and r["stats"][1] == 0, r["stats"]
            _check_exact(r, exp, "gather path%s" % (" in passes" if p == 2 else ""))
        _check_exact(runs[p][1], runs[p][0], "run to run")
    for r in runs[1]:
        assert r["stats"] is None                                        # (the gather kernel did not run)
        _check_bars(r, exp, "two-pass path")
    _check_same_class(runs[1][0], runs[1][1], "two-pass path, run to run")


@pytest.mark.parametrize("valid,occlude,out_half", [(True, True, False), (False, False, False), (True, False, True), (False, True, True)])
def test_fp16_splat_follows_rule_g(valid, occlude, out_half, dev, native):
    """Flow and 2 data channels stored in fp16 (ofl_splat_tiled_f16) at 64 x 96, with the fp16 specials: the `_Float16` kernels against
    the restatement on the exact fp32 up-conversions (an fp16 result: its fp32 values rounded to fp16); the two-pass route, which
    up-converts, against the same on its bars."""
    h, w, c = 64, 96, 2
    case = sv.make_splat(h, w, c, half=True)
    o = dict(masked=True, mch=(True, False) if valid else None, occlude=occlude, sign=1.0, want=dict(want_valid=True) if valid else {})
    exp = _expected(h, w, c, True, o)
    exp = dict(v=exp["v"], m=exp["m"], den=None, warped=None, scale=exp["scale"])
    with np.errstate(over="ignore"):
        exp16 = dict(exp, v=exp["v"].astype(np.float16)) if out_half else exp
    runs = [_on_path(native, 0, lambda: _splat_call(native, dev, case, o, half=True, out_half=out_half)) for _ in range(2)]
    for r in runs:
        assert "DF16_" in r["kernel"], r["kernel"]
        assert r["stats"][0] == 0 and r["stats"][1] == 0, r["stats"]
        _same(r["v"], exp16["v"], "fp16 gather path")
        if valid:
            assert np.array_equal(r["m"], exp["m"])
    _same(runs[1]["v"], runs[0]["v"], "run to run")
    two = _on_path(native, 1, lambda: _splat_call(native, dev, case, o, half=True))
    _check_bars(dict(v=two["v"], m=two["m"]), dict(exp, den=None, warped=None), "fp16 inputs on the two-pass path")
    assert np.array_equal(sv.classes(two["v"]), sv.classes(runs[0]["v"].astype(np.float32))) or out_half


@pytest.mark.parametrize("h,w,c", sv.SPLAT_FRAMES)
def test_splat_sum_follows_rule_g(h, w, c, dev, native):
    """_native.splat_sum (the transpose of the backward warp: undivided sums at the positions the warp samples) on the same inputs,
    against the restatement under rule G, bit for bit, twice."""
    case = sv.make_splat(h, w, c)
    exp = sv.splat_sum_restated(case["flow"], case["data"])
    f, d = torch.from_numpy(case["flow"]).to(dev), torch.from_numpy(case["data"]).to(dev)
    outs = []
    for _ in range(2):
        native._last_splat_stats = None
        out = native.splat_sum(f, d, flow_sign=-1.0)
        assert out is not None
        st = native._last_splat_stats.cpu().tolist()
        assert st[0] == 0 and st[1] == 0, st
        outs.append(out.cpu().numpy())
        _same(outs[-1], exp, "splat_sum")
    _same(outs[1], outs[0], "run to run")


def test_splat_sum_follows_rule_g_where_the_image_falls_back(dev, native):
    """_native.splat_sum of a flow that draws the frame into a fifth of its area (256 x 384, as the queue-capacity case of
    tests/test_gpu_parity.py): the image's lists overflow and the call sums it with the two-pass kernel's float atomics in raw mode.
    Specials on pixels whose sample position is an integer that survives the normalisation (three corners of weight 0 each): classes
    as rule G exactly, finite elements on the bars (absolute part from the finite background), twice with the same classes."""
    n, c, h, w = 1, 2, 256, 384
    rng = np.random.default_rng(8)
    data = (rng.integers(-512, 512, size=(n, c, h, w)) / 64.0).astype(np.float32)
    flow = np.empty((n, 2, h, w), np.float32)
    flow[0, 0] = np.float32(0.8) * (np.arange(w, dtype=np.float32)[None, :] - np.float32(190.3))
    flow[0, 1] = np.float32(0.8) * (np.arange(h, dtype=np.float32)[:, None] - np.float32(120.7))
    ex, ey = sv.exact_coords(w), sv.exact_coords(h)
    bg = data.copy()
    for i in range(12):
        y, x = 11 + 19 * i, 17 + 29 * i
        tx, ty = sv._nearest(ex, 150 + 7 * i), sv._nearest(ey, 100 + 4 * i)
        flow[0, :, y, x] = (x - tx, y - ty)
        data[0, :, y, x] = sv.NONFINITE[i % 3]
    exp = sv.splat_sum_restated(flow, data)
    assert (sv.classes(exp) != sv.classes(sv.splat_sum_restated(flow, data, sv.NONZERO))).sum() >= 24      # (zero-weight corners tell)
    scale = sv.background_scale(dict(v=sv.splat_sum_restated(flow, bg)))
    f, d = torch.from_numpy(flow).to(dev), torch.from_numpy(data).to(dev)
    outs = []
    for _ in range(2):
        native._last_splat_stats = None
        out = native.splat_sum(f, d, flow_sign=-1.0)
        assert out is not None
        st = native._last_splat_stats.cpu().tolist()
        assert st[0] != 0, st                                            # the image took the two-pass path inside the call
        outs.append(dict(v=out.cpu().numpy()))
        _check_bars(outs[-1], dict(v=exp, m=None, den=None, warped=None, scale=scale), "splat_sum on the fallback")
    _check_same_class(outs[1], outs[0], "run to run")


# ---- folded bands and planned bands (frames of tests/splat_cells.py) ---------------------------------------------------------------
def _cells_case(kind):
    """A frame of splat_cells.make(kind) with specials planted on sources of chosen cells: the longest cell of each destination tile
    (in 'fold': the cells of 65 and 80 records, inside the folded bands), a cell of 3 ... 8 records of each tile (outside them), and on
    one source of each the end point moved on to the cell's corner (integer end point: three corners of weight 0).  planted: (b, Y, X) of
    the destination cells, one entry per special."""
    fr, info, data, ca = sc.make(kind)
    flow, data = fr.flow.copy(), data[:, :3].copy()
    planted = []
    for b, ty, tx in info["tiles"]:
        cells = [(k, key) for key, (k, z) in fr.cells.items() if key[0] == b and key[1] // sc.TW == tx and not z]
        long_ = max(cells)[1]
        short = min((k, key) for k, key in cells if k >= 3)[1]
        for j, key in enumerate((long_, short)):
            srcs = fr.records(key)
            for i, (sx, sy) in enumerate((srcs[0], srcs[-1])):
                for ch in range(3):
                    data[b, ch, sy, sx] = sv.NONFINITE[(i + j + ch + b + tx) % 3]
                if i == 0:
                    flow[b, 0, sy, sx], flow[b, 1, sy, sx] = key[1] - sx, key[2] - sy
                planted.append((b, key[2], key[1]))                        # (the destination cell's first pixel: b, Y, X)
    return fr, info, flow, data, ca, planted


@pytest.mark.parametrize("kind", ["fold", "second"])
def test_specials_in_folded_and_planned_bands(kind, dev, native):
    """'fold': tiles whose marked bands are summed with LDS float atomics, specials inside and outside the bands; 'second': tiles of more
    records than the LDS holds, summed in planned bands by the second launch.  Outside the marked bands rule G bit for bit, inside on
    the bars; classes and masks exactly everywhere; the two-pass path gives every element the same class."""
    import test_gpu_splat_cells as tc
    fr, info, flow, data, ca, planted = _cells_case(kind)
    assert len(planted) >= 8 and sc.record_counts(flow, fr.on, True) == fr.counts(True)       # (moving an end point inside its cell keeps the counts)
    dd = np.concatenate([data, ca[:, None].astype(np.float32)], 1)
    out, warped, den = sv.splat_restated(flow, dd, fr.on, True, sv.G)
    exp = dict(v=out[:, :3], m=out[:, 3], den=den, warped=warped)
    assert not np.isfinite(exp["v"]).all()
    # the tolerance's absolute part: from the same flow over the frame's own finite data (special_values.background_scale)
    bg = np.concatenate([sc.make(kind)[2][:, :3], ca[:, None].astype(np.float32)], 1)
    out, warped, den = sv.splat_restated(flow, bg, fr.on, True, sv.G)
    exp["scale"] = sv.background_scale(dict(v=out[:, :3], m=out[:, 3], den=den))
    kw = dict(weight_mask=torch.from_numpy(fr.on).to(dev), chan_mask_a=torch.from_numpy(ca).to(dev), want_mask_chan=True, want_density=True,
              want_warped=True)
    f, d = torch.from_numpy(flow).to(dev), torch.from_numpy(data).to(dev)

    def call():
        o = native.splat_fwd(f, d, **kw)
        return dict(v=_np(o[0]), m=_np(o[1]), den=_np(o[2]), warped=_np(o[3]), stats=native._last_splat_stats.cpu().tolist(),
                    ws=native._last_splat_ws.cpu().numpy())

    runs = [_on_path(native, 0, call) for _ in range(2)]
    for r in runs:
        st = r["stats"]
        units = sc.redo_units(r["ws"], fr.n, fr.h, fr.w, native.splat_tile_geometry()[2])
        assert st[0] == 0 and st[2] == 0 and st[3] > 0, st
        marked = [u for u in units if u[5]]
        assert (len(marked) > 0 and st[1] == len(marked)) if kind == "fold" else (marked == [] and st[1] == 0), (st, marked)
        allowed = tc._allowed(units, fr, marked)
        bad = np.zeros_like(allowed)
        for key in ("v", "m", "den", "warped"):
            miss = ~sv.same_bits(r[key], exp[key])
            bad |= miss.any(1) if miss.ndim == 4 else miss
        assert not (bad & ~allowed).any(), "%d pixels outside the folded bands differ from rule G: %s" % (
            int((bad & ~allowed).sum()), np.argwhere(bad & ~allowed)[:6].tolist())
        _check_bars(r, exp, kind)
        if kind == "fold":                                              # (specials on both sides of the band boundaries)
            inside = [p for p in planted if allowed[p]]
            assert 0 < len(inside) < len(planted)
    if kind == "second":
        _check_exact(runs[1], runs[0], "run to run")
    _check_same_class(runs[1], runs[0], "run to run")
    native.collect_splat_stats = True
    two = _on_path(native, 1, lambda: dict(zip(("v", "m", "den", "warped"), (_np(t) for t in native.splat_fwd(f, d, **kw)))))
    _check_bars(two, exp, "two-pass path")
    _check_same_class(two, runs[0], "two-pass path against the gather path")


# ---- the API --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'specials.npz')) as z:
        return {k: z[k] for k in z.files}


def test_api_s_follows_rule_g_on_the_fixture_inputs(fx, dev):
    """apply_flow 's' and Flow.apply 's' on the reference fixture's inputs (24 x 36): rule G, i.e. the restatement under G -- NOT the
    fixture's outputs, which follow the reference's ALL; where the two rules agree the fixture's bits are asserted too."""
    import oflibpytorch_amd as ofl
    from oracle import oracle
    f, d, m, ca = fx["s_flow"], fx["s_data"], fx["s_mask"], fx["s_ca"]
    tf, td, tm, tca = (torch.from_numpy(a).to(dev) for a in (f, d, m, ca))
    for mask, key in ((m, "s_apply_flow_masked"), (None, "s_apply_flow_unmasked")):
        got = ofl.apply_flow(tf, td, 's', None if mask is None else tm).cpu().numpy()
        exp = sv.splat_restated(f, d, mask, True, sv.G)[0]
        _same(got, exp, "apply_flow 's'")
        agree = sv.same_bits(exp, fx[key])
        assert agree.sum() > agree.size // 2 and not agree.all()
        assert sv.same_bits(got, fx[key])[agree].all()
    got, valid = ofl.Flow(tf, 's', tm).apply(td, target_mask=tca, return_valid_area=True)
    dd = np.concatenate([d, (ca & m)[:, None].astype(np.float32)], 1)
    exp = sv.splat_restated(f, dd, m, True, sv.G)[0]
    _same(got.cpu().numpy(), exp[:, :3], "Flow.apply 's'")
    assert np.array_equal(valid.cpu().numpy(), oracle.theta(exp[:, 3]))


def test_api_t_equals_the_reference_fixture(fx, dev):
    """apply_flow 't' and Flow.apply 't' at 24 x 36 against the reference's own results."""
    import oflibpytorch_amd as ofl
    tf, ts = torch.from_numpy(fx["t_flow"]).to(dev), torch.from_numpy(fx["t_src"]).to(dev)
    _same(ofl.apply_flow(tf, ts, 't').cpu().numpy(), fx["t_apply_flow"], "apply_flow 't'")
    got, valid = ofl.Flow(tf, 't', torch.from_numpy(fx["t_mask"]).to(dev)).apply(ts, target_mask=torch.from_numpy(fx["t_tmask"]).to(dev),
                                                                                return_valid_area=True)
    _same(got.cpu().numpy(), fx["t_flow_apply"], "Flow.apply 't'")
    assert np.array_equal(valid.cpu().numpy(), fx["t_flow_apply_valid"])


# ====================================================================================================================================
# the warp
# ====================================================================================================================================
def _warp_cases():
    """One case per distinct recorded kernel name of the fp32 ('plain') and fp16-source ('half') kinds: the smallest launch that
    reaches the kernel."""
    import test_gpu_warp_kernel_choice as kc
    by = {}
    for case in kc.CASES:
        if case["kind"] in ("plain", "half"):
            by.setdefault((case["kind"], kc.RECORDED[case["id"]]), []).append(case)
    picked = [min(cs, key=lambda c: (c["n"] * c["h"] * c["w"] * c["c"], c["id"])) for cs in by.values()]
    return sorted(picked, key=lambda c: (c["n"], c["h"], c["w"], c["kind"], c["id"]))


_WARP = {}


def _warp_data(n, h, w, half):
    """flow, 8 source planes, 3 planes of another field (specials sprinkled too), a mask -- cached per shape, NumPy and device."""
    key = (n, h, w, half)
    if key not in _WARP:
        if len(_WARP) >= 2:
            _WARP.pop(next(iter(_WARP)))
        t = sv.warp_case(n, h, w, 8, seed=1, half=half)
        rng = np.random.default_rng(n + h + w)
        other = (rng.integers(-256, 256, size=(n, 3, h, w)) / 32.0).astype(np.float32)
        hit = rng.random(other.shape) < 0.02
        other[hit] = np.array([sv._plant_cycle(i, False) for i in range(7)], np.float32)[np.arange(int(hit.sum())) % 7]
        mask = rng.random((n, h, w)) > 0.15
        _WARP[key] = (t, other, mask)
    return _WARP[key]


def _warp_expected(flow, src, kw_np):
    """dst and valid of one warp_bwd call from oracle.G: the mask channel rides as one more source channel."""
    from oracle import oracle
    c = src.shape[1]
    with np.errstate(all="ignore"):
        s = src if kw_np.get("src_b") is None else src - kw_np["src_b"]
    if kw_np.get("valid"):
        s = np.concatenate([s, kw_np["mask"][:, None].astype(np.float32)], 1)
    g = oracle.G(flow, s)
    exp = g[:, :c]
    if kw_np.get("addend") is not None:
        with np.errstate(all="ignore"):
            exp = np.float32(1.0) * kw_np["addend"] + np.float32(-1.0) * exp
    valid = (oracle.theta(g[:, c]) & kw_np["mask"]) if kw_np.get("valid") else None
    # the valid area of the same flow and masks over an all-zero image: a non-finite image must not move it
    if valid is not None:
        z = np.concatenate([np.zeros_like(src[:, :1]), kw_np["mask"][:, None].astype(np.float32)], 1)
        assert np.array_equal(valid, oracle.theta(oracle.G(flow, z)[:, 1]) & kw_np["mask"])
    return exp, valid


@pytest.mark.parametrize("case", _warp_cases(), ids=lambda c: c["id"])
def test_warp_kernels_carry_specials_as_the_reference(case, dev, native):
    """Specials in the source (and in the addend), flow components of +-3.4e38, +-1e-42, 2^24 and 2^31, samples on integers, on the
    last row and column, at -1, 0, w - 1 and w: `_native.warp_bwd` against oracle.G bit for bit, the valid area against oracle.theta
    exactly, the kernel the recorded one, the output's flag word equal to a flag pass over the stored output."""
    import test_gpu_warp_kernel_choice as kc
    n, h, w, c, half = case["n"], case["h"], case["w"], case["c"], case["kind"] == "half"
    t, other, mask = _warp_data(n, h, w, half)
    flow, src = t["flow"], np.ascontiguousarray(t["src"][:, :c])
    kw, kn = {}, {}
    tmask = torch.from_numpy(mask).to(dev)
    tflow = torch.from_numpy(flow).to(dev)
    if case.get("valid"):
        kw.update(want_valid=True, src_mask=tmask, flow_mask=tmask)
        kn.update(valid=True, mask=mask)
    if case.get("addend"):
        add = flow if case["addend"] == "flow" else np.ascontiguousarray(other[:, :c])
        kw.update(addend=tflow if case["addend"] == "flow" else torch.from_numpy(add).to(dev), a_sign=1.0, g_sign=-1.0)
        kn["addend"] = add
    if case.get("dst_flags"):
        kw["want_dst_flags"] = True
    if case.get("flags"):
        kw.update(want_flags=True, want_src_flags=case["flags"] == "src")
    if case.get("src_b"):
        with np.errstate(all="ignore"):
            kn["src_b"] = np.ascontiguousarray(other[:, :2] * np.float32(30))
        kw["src_b"] = torch.from_numpy(kn["src_b"]).to(dev)
    tsrc = torch.from_numpy(src)
    if half:
        tsrc = tsrc.half()
        assert torch.equal(tsrc.float().nan_to_num(3.0), torch.from_numpy(src).nan_to_num(3.0))
    native.set_warp_path(case["path"])
    try:
        res = native.warp_bwd(tflow, tsrc.to(dev), **kw)
        raw = native.last_kernel_name(demangle=False)
        if raw not in kc._NAMES:                                         # (demangled once per kernel, as in that file)
            kc._NAMES[raw] = native.last_kernel_name()
        name = kc._NAMES[raw]
    finally:
        native.set_warp_path(0)
    assert name == kc.RECORDED[case["id"]]
    exp, valid = _warp_expected(flow, src, kn)
    _same(res[0].cpu().numpy(), exp, "warped values")
    if valid is not None:
        assert np.array_equal(res[1].cpu().numpy(), valid)
    if case.get("dst_flags"):
        assert torch.equal(res[4], native.flow_flags(res[0], res[1]))
    assert not np.isfinite(exp).all() and np.isfinite(exp).sum() > exp.size // 2


def test_oversize_box_carries_specials_as_the_reference(dev, native):
    """The stretch of test_oversize_boxes_staged_in_part_stay_exact at its smallest frame (100 x 330, 3.5: boxes larger than the LDS
    budget, staged in part), one channel, specials sprinkled over the source: the column kernel and the generic kernel against the
    oracle on the first and last images, and against each other on all."""
    from oracle import oracle
    h, w, stretch = 100, 330, 3.5
    n = 6912 // (((w + 31) // 32) * ((h + 63) // 64)) + 1
    t = sv.warp_case(n, h, w, 1, seed=2, sprinkle=0.01)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    flow = t["flow"] * np.float32(0.25)
    named = np.zeros((h, w), bool)
    for where in t["names"].values():
        for y, x in where:
            named[y, x] = True
    flow[:, 0] = np.where(named, t["flow"][:, 0], flow[:, 0] - (xs - w / 2) * np.float32((stretch - 1.0) * 0.8))
    flow[:, 1] = np.where(named, t["flow"][:, 1], flow[:, 1] - (ys - h / 2) * np.float32(stretch - 1.0))
    tf, ts = torch.from_numpy(flow).to(dev), torch.from_numpy(t["src"]).to(dev)
    outs = {}
    for path in (0, 1):
        native.set_warp_path(path)
        try:
            outs[path] = native.warp_bwd(tf, ts)[0].cpu().numpy()
            name = native.last_kernel_name()
        finally:
            native.set_warp_path(0)
        if path == 0:
            assert "warp_bwd_lds_column_kernel<4," in name, name
    pick = [0, 1, n - 1]
    exp = oracle.G(flow[pick], t["src"][pick])
    assert not np.isfinite(exp).all()
    _same(outs[0][pick], exp, "column kernel")
    _same(outs[1], outs[0], "generic kernel against the column kernel")


# ====================================================================================================================================
# the side kernel
# ====================================================================================================================================
@pytest.mark.parametrize("scale", [0.5, 1.7])
def test_resize_bilinear_carries_specials(scale, dev, native):
    """resize_bilinear at 9 x 13 with a NaN and an infinity in the source against oracle.resize_bilinear, bit for bit."""
    from oracle import oracle
    rng = np.random.default_rng(3)
    x = (rng.integers(-512, 512, size=(2, 3, 9, 13)) / 64.0).astype(np.float32)
    x[0, 0, 4, 6], x[0, 1, 2, 3], x[1, 2, 8, 12], x[1, 0, 0, 0] = np.nan, np.inf, -np.inf, sv.FLT_MAX
    x[1, 1, 5, 5], x[0, 2, 7, 1] = sv.DEN_MIN, -0.0
    exp = oracle.resize_bilinear(x, [scale, scale])
    got = native.resize_bilinear(torch.from_numpy(x).to(dev), [scale, scale]).cpu().numpy()
    k = sv.classes(exp)
    assert (k == 1).any() and (k != 0).sum() < k.size // 2
    _same(got, exp, "resize_bilinear x %g" % scale)
