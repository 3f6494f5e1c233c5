"""GPU tier: every recorded kernel of the backward warp on every swept frame it can reach (tests/frame_sweep.py: the frame lines, their
content, the batch that keeps a frame in a kernel's size class; tests/test_frame_sweep_host.py pins those on the CPU).

One parametrised test per distinct kernel name of tests/golden/warp_kernel_choice.json (kinds plain, u8, half, grad, the channel loop
and the launches split into groups of 3 channels) and per entry of the 16-bit table of tests/test_gpu_half_warp.py, fp16 and bf16; the
frames are looped inside.  Per launch: `last_kernel_name()` is the recorded name of the base case (the table is not re-recorded), and
  plain, half   dst == oracle.G bit for bit (addend and src_b as in test_gpu_special_values._warp_expected), valid == oracle.theta, the
                output's flag word == a flag pass over the stored output, the flow's flag word == a flag pass over the flow;
  u8            the oracle, rounded half to even and clamped where the launch rounds;
  grad          inside the per-element bound of tests/grad_oracle64.py, nothing excluded;
  16-bit        the raw 16-bit patterns of the fp32 route (oracle.G of the up-converted source, converted once).
A launch of n images is the frame's four images repeated cyclically, compared ON THE DEVICE with the four expected images repeated; a
failure names the frame, the batch and the first differing (n, c, y, x).  The generic kernel (path 1) runs first, on every frame of
both lines, widths 2 and 3 included, which no staged kernel takes."""
import numpy as np
import pytest
import torch

import frame_sweep as fs
import grad_oracle64 as g64

pytestmark = pytest.mark.gpu

RECORDED = fs.recorded_cases()
X16 = fs.x16_cases()
REACHED = {}          # kernel -> the frames it ran on in this process (the last test prints it; nothing is asserted on it)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tier needs a HIP device"
    from oflibpytorch_amd import _native
    _native.load_library()
    return torch.device('cuda', 0)


@pytest.fixture
def native():
    from oflibpytorch_amd import _native
    yield _native
    _native.set_warp_path(0)


_DEV, _EXP = {}, {}


def _frame(h, w, dev):
    """The frame's content on the device (four images)."""
    if (h, w) not in _DEV:
        t = fs.content(h, w)
        _DEV[(h, w)] = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in t.items() if isinstance(v, np.ndarray)}
    return _DEV[(h, w)]


def _opt_key(case):
    return (case["kind"], case["c"], bool(case.get("valid")), case.get("addend"), bool(case.get("src_b")), bool(case.get("to_u8")),
            str(case.get("dtype")))


def _source(t, case):
    """The four source images of a case as the kernel reads them, in fp32 (exactly: integers 0 ... 255, / 16 for the 16-bit kinds)."""
    src = np.ascontiguousarray(t["src"][:, :case["c"]])
    return src / np.float32(16) if case["kind"] in ("half", "x16") else src


def _expected(h, w, case, dev):
    """(dst, valid | None) of the frame's four images from the oracle, on the device (cached per frame and option set); for the
    gradient (value, bound) in fp64."""
    from oracle import oracle
    key = (h, w) + _opt_key(case)
    if key in _EXP:
        return _EXP[key]
    t = fs.content(h, w)
    c, kind = case["c"], case["kind"]
    src = _source(t, case)
    if kind == "grad":
        gout = np.ascontiguousarray(t["src"][:, 9 - c:] - np.float32(100))
        val, M, k = g64.warp_grad(t["flow"], src, gout, 1.0, 0.5)["grad_flow"]
        out = (torch.from_numpy(val).to(dev), torch.from_numpy(g64.bound(M, k, g64.R["warp.grad_flow"])).to(dev))
        _EXP[key] = out
        return out
    s = src - t["other"][:, :2] * np.float32(30) if case.get("src_b") else src
    if case.get("valid"):
        s = np.concatenate([s, t["m1"][:, None].astype(np.float32)], 1)
    g = oracle.G(t["flow"], s)
    exp = g[:, :c]
    if case.get("addend"):
        add = t["flow"] if case["addend"] == "flow" else t["other"][:, :c]
        exp = np.float32(1.0) * add + np.float32(-1.0) * exp
    if case.get("to_u8"):
        exp = np.clip(np.rint(exp), 0, 255).astype(np.uint8)              # torch.round (half to even) + clamp
    exp = torch.from_numpy(np.ascontiguousarray(exp))
    if kind == "x16":
        exp = exp.to(case["dtype"])                                       # (the fp32 route's result, converted once)
    valid = torch.from_numpy(oracle.theta(g[:, c]) & t["m2"]).to(dev) if case.get("valid") else None
    _EXP[key] = (exp.to(dev), valid)
    return _EXP[key]


def _launch(native, case, h, w, n, dev):
    """The base case's call on n images of the frame -> (results, raw kernel name)."""
    d = _frame(h, w, dev)
    c, kind = case["c"], case["kind"]
    flow = fs.batch(d["flow"], n)
    src = fs.batch(d["src"][:, :c], n).contiguous()
    kw = {}
    if case.get("valid"):
        kw.update(want_valid=True, src_mask=fs.batch(d["m1"], n), flow_mask=fs.batch(d["m2"], n))
    native.set_warp_path(case["path"])
    try:
        if kind == "grad":
            gout = fs.batch(d["src"][:, 9 - c:] - 100, n).contiguous()
            res = native.warp_bwd_grad(flow, src, gout, g_scale=0.5, want_src=False)[1:]
        elif kind == "x16":
            res = native._warp_bwd_x16(flow, (src / 16).to(case["dtype"]), **kw)
            assert res is not None, "the library declined the 16-bit launch"
        else:
            if case.get("addend"):
                kw.update(addend=flow if case["addend"] == "flow" else fs.batch(d["other"][:, :c], n).contiguous(), a_sign=1.0, g_sign=-1.0)
            if case.get("dst_flags"):
                kw.update(want_dst_flags=True)
            if case.get("flags"):
                kw.update(want_flags=True, want_src_flags=case["flags"] == "src")
            if case.get("src_b"):
                kw.update(src_b=fs.batch(d["other"][:, :2] * 30, n).contiguous())
            if kind == "plain":
                res = native.warp_bwd(flow, src, **kw)
            elif kind == "half":
                res = native.warp_bwd(flow, (src / 16).half(), **kw)
            else:
                rm = native.ROUND_U8 if case.get("to_u8") else native.ROUND_NONE
                res = native.warp_bwd(flow, src.to(torch.uint8), round_mode=rm, out_uint8=bool(case.get("to_u8")), **kw)
        raw = native.last_kernel_name(demangle=False)
    finally:
        native.set_warp_path(0)
    return res, raw, flow, kw


_BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.uint8: torch.uint8, torch.bool: torch.bool}


def _first_difference(got, exp4):
    """None, or a description of the first element of `got` [n, ...] whose bits differ from the four expected images repeated."""
    n = got.shape[0]
    assert got.dtype == exp4.dtype and got.shape[1:] == exp4.shape[1:], (got.dtype, exp4.dtype, got.shape, exp4.shape)
    exp = fs.batch(exp4, n)
    bad = got.contiguous().view(_BITS[got.dtype]) != exp.contiguous().view(_BITS[got.dtype])
    count = int(bad.sum())
    if not count:
        return None
    idx = tuple(int(i) for i in torch.nonzero(bad)[0])
    return "%d of %d elements differ, the first at %s: got %r, expected %r" % (count, bad.numel(), idx, got[idx].item(), exp[idx].item())


def _first_excess(got, val4, bound4):
    """None, or the first element of the gradient outside its bound."""
    n = got.shape[0]
    val, bnd = fs.batch(val4, n), fs.batch(bound4, n)
    bad = ~((got.double() - val).abs() <= bnd)                             # (a NaN is outside)
    count = int(bad.sum())
    if not count:
        return None
    idx = tuple(int(i) for i in torch.nonzero(bad)[0])
    return "%d of %d elements outside the bound, the first at %s: got %r, fp64 value %r, bound %.3g" % (
        count, bad.numel(), idx, got[idx].item(), val[idx].item(), bnd[idx].item())


def _check(native, case, h, w, n, dev, res, flow, kw):
    where = "frame %d x %d, n %d (%s)" % (h, w, n, case.get("id", case["kind"]))
    exp = _expected(h, w, case, dev)
    if case["kind"] == "grad":
        msg = _first_excess(res[0], *exp)
        assert msg is None, "%s, gradient wrt the flow: %s" % (where, msg)
        return
    want = exp[0]
    if case.get("to_u8") and res[0].dtype == torch.float32:              # no uint8 store on this route (the generic kernel): the rounded values in fp32
        want = want.float()
    msg = _first_difference(res[0], want)
    assert msg is None, "%s, warped values (n, c, y, x): %s" % (where, msg)
    if case.get("valid"):
        msg = _first_difference(res[1], exp[1])
        assert msg is None, "%s, valid area (n, y, x): %s" % (where, msg)
    else:
        assert res[1] is None
    if case.get("dst_flags"):
        assert torch.equal(res[4], native.flow_flags(res[0], res[1])), "%s: the output's flag word" % where
    if case.get("flags"):
        assert torch.equal(res[2], native.flow_flags(flow, kw.get("flow_mask"))), "%s: the flow's flag word" % where


_DEMANGLED = {}


def _name(native, raw):
    if raw not in _DEMANGLED:                                             # (the last launch is still the one named `raw`)
        _DEMANGLED[raw] = native.last_kernel_name()
    return _DEMANGLED[raw]


# ---- the generic kernel first -------------------------------------------------------------------------------------------------------
GENERIC = [dict(kind="plain", c=3, path=fs.GENERIC, valid=True), dict(kind="plain", c=2, path=fs.GENERIC, valid=True, addend="flow", dst_flags=True),
           dict(kind="plain", c=2, path=fs.GENERIC, valid=True, src_b=True), dict(kind="plain", c=1, path=fs.GENERIC, addend="other"),
           dict(kind="u8", c=3, path=fs.GENERIC, valid=True, to_u8=True), dict(kind="grad", c=2, path=fs.GENERIC)]


@pytest.mark.parametrize("case", GENERIC, ids=lambda c: "-".join("%s%s" % (k, "" if v is True else v) for k, v in sorted(c.items())))
def test_generic_kernel_on_every_frame(case, dev, native):
    """Path 1 (and every frame narrower than 4, whatever the path): the direct-gather kernels, 13 images (three rounds of the four
    and one more) of every frame of both lines."""
    for h, w in fs.FRAMES:
        res, raw, flow, kw = _launch(native, case, h, w, 13, dev)
        name = _name(native, raw)
        # (the generic kernel leaves the output's flag word to a flag pass of its own: that launch is then the last)
        assert "warp_bwd_kernel" in name or "warp_grad" in name or (case.get("dst_flags") and "flow_flags_kernel" in name), "frame %d x %d: %s" % (h, w, name)
        _check(native, case, h, w, 13, dev, res, flow, kw)


# ---- every recorded kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,case", RECORDED, ids=[c["id"] for _, c in RECORDED])
def test_recorded_kernel_on_every_frame_it_reaches(name, case, dev, native):
    frames = fs.frames_for(case)
    assert not fs.residue_gaps(case, frames)
    for h, w, n in frames:
        res, raw, flow, kw = _launch(native, case, h, w, n, dev)
        got = _name(native, raw)
        assert got == name, "frame %d x %d, n %d (%s): launched %s" % (h, w, n, case["id"], got)
        _check(native, case, h, w, n, dev, res, flow, kw)
    REACHED[(case["kind"], name)] = frames


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("key,base", X16, ids=["%s-%d-c%d-%s" % (k[0], k[1], k[2], "valid" if k[3] else "plain") for k, _ in X16])
def test_16_bit_kernel_on_every_frame_it_reaches(key, base, dtype, dev, native):
    import test_gpu_half_warp as hw
    case = dict(base, dtype=dtype)
    frames = fs.frames_for(base)
    assert not fs.residue_gaps(base, frames)
    for h, w, n in frames:
        res, raw, flow, kw = _launch(native, case, h, w, n, dev)
        got = hw._key(_name(native, raw))
        assert got == (key, dtype), "frame %d x %d, n %d: launched %s" % (h, w, n, _name(native, raw))
        _check(native, case, h, w, n, dev, res, flow, kw)
    REACHED[("x16 %s" % dtype, str(key))] = frames


# ---- the API ---------------------------------------------------------------------------------------------------------------------------
def test_api_line_at_batch_2(dev):
    """Flow.apply 't', combine_with mode 3 and switch_ref (both references) at B = 2 on the width line at H = 17, against the oracle."""
    import oflibpytorch_amd as ofl
    from oracle import oracle
    for h, w in fs.WIDTH_LINE:
        if h != 17:
            continue
        t, d = fs.content(h, w), _frame(h, w, dev)
        f1, f2, m1, m2, img = t["flow"][:2], t["flow"][2:], t["m1"][:2], t["m2"][2:], np.ascontiguousarray(t["src"][:2, :3])
        F1, F2 = ofl.Flow(d["flow"][:2], 't', d["m1"][:2]), ofl.Flow(d["flow"][2:], 't', d["m2"][2:])
        where = "frame %d x %d" % (h, w)
        warped, valid = F2.apply(d["src"][:2, :3].contiguous(), target_mask=d["m1"][:2], return_valid_area=True)
        ow, ov = oracle.flow_apply(f2, 't', m2, img, m1)
        assert np.array_equal(warped.cpu().numpy().view(np.uint32), ow.view(np.uint32)), "%s: Flow.apply 't'" % where
        assert np.array_equal(valid.cpu().numpy(), ov), "%s: Flow.apply 't', valid area" % where
        f3 = F1.combine_with(F2, 3)
        o3, om3, _ = oracle.combine_with(f1, m1, f2, m2, 3, 't')
        assert np.array_equal(f3.vecs.cpu().numpy().view(np.uint32), o3.view(np.uint32)), "%s: combine_with mode 3" % where
        assert np.array_equal(f3.mask.cpu().numpy(), om3), "%s: combine_with mode 3, mask" % where
        for ref in "st":
            out = ofl.Flow(d["flow"][:2], ref, d["m1"][:2]).switch_ref()
            exp, expm, _ = oracle.switch_ref(f1, ref, m1)
            if w >= 4:
                assert np.array_equal(out.vecs.cpu().numpy(), exp), "%s: switch_ref from '%s'" % (where, ref)
            else:                                                         # no gather path under 4 columns: float atomics, the two-pass bar
                np.testing.assert_allclose(out.vecs.cpu().numpy(), exp, rtol=2e-5, atol=2e-5 * float(np.abs(exp).max()),
                                           err_msg="%s: switch_ref from '%s'" % (where, ref))
            assert np.array_equal(out.mask.cpu().numpy(), expm), "%s: switch_ref from '%s', mask" % (where, ref)


def test_zz_the_table_of_what_runs_where():
    """Prints, per kernel of both tables, the frames it is run on and the residues of W and H among them -- computed from
    `frame_sweep.frames_for`, what the tests above loop over, so it does not depend on which of them ran -- and whether this process ran
    it.  Every name of both tables is in it; the residue condition itself is asserted per kernel above and in the CPU tier."""
    import test_gpu_warp_kernel_choice as kc
    rows = [((case["kind"], name), case) for name, case in RECORDED]
    rows += [(("x16 %s" % dt, str(key)), base) for key, base in X16 for dt in (torch.float16, torch.bfloat16)]
    for (kind, name), case in sorted(rows, key=lambda r: r[0]):
        frames = fs.frames_for(case)
        print("%-6s %3d frames  W %% 64 in %s  H %% 64 in %s  %s  %s" % (kind[:6], len(frames), sorted({w % 64 for _, w, _ in frames}),
                                                                          sorted({h % 64 for h, _, _ in frames}), name,
                                                                          "ran" if (kind, name) in REACHED else "not run in this process"))
        assert frames and not fs.residue_gaps(case, frames)
    assert {key for key, _ in rows if not key[0].startswith("x16")} == {(c["kind"], kc.RECORDED[c["id"]]) for c in kc.CASES}
