"""GPU tier (`pytest -m gpu`, real MI355X): the package's public API running on the HIP kernels (through the
C ABI) must reproduce what the reference produced.

Bars (BASELINE.json north_star):
  * backward-gather ('t') family -- the kernel restates the reference's fp32 operation order, so values AND
    masks are compared BIT-EXACT;
  * forward-splat ('s') family -- the gather kernel (C <= 3, W >= 4: every fixture but the 2 x 2 one) sums each destination pixel's
    contributions in the reference's own order, so values AND masks are compared BIT-EXACT as well; the general two-pass
    path (float atomics; C > 3) is held to rtol 2e-5 / atol 2e-5 * max|expected| with masks bit for bit (tests below).
"""
import numpy as np
import pytest
import torch

from conftest import golden_ids
import case_runner

pytestmark = pytest.mark.gpu

ALL = [c for c in golden_ids() if not c.endswith("cfg1_inputs") and not c.startswith("gen.")]   # (group gen: tests/test_gpu_generators.py)


def uses_splat(case):
    op, a = case["op"], case["args"]
    ref = a.get("ref")
    if op in ('grid_from_unstructured_data', 'apply_s_flow', 'kat_gfud', 'Flow.switch_ref', 'switch_flow_ref'):
        return a.get("mode") != "invalid"
    if op in ('apply_flow', 'Flow.apply'):
        return ref == 's'
    if op == 'Flow.invert':
        return (a["arg_ref"] or ref) == ref
    if op == 'invert_flow':
        return (a["out_ref"] or ref) == ref
    if op in ('Flow.combine_with', 'combine_flows'):
        return a["mode"] in (1, 2)
    if op == 'Flow.valid_target':
        return ref == 's'
    if op == 'Flow.valid_source':
        return ref == 't'
    if op == 'kat_cfg1':
        return a["call"] == 'switch_ref' or (a["call"] == 'apply' and ref == 's') or a.get("mode") in (1, 2)
    if op == 'Flow.combine':
        return True
    if op in ('track_pts', 'Flow.track'):
        return ref == 't'
    return False


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tier needs a HIP device"
    from oflibpytorch_amd import _native
    _native.load_library()
    return torch.device('cuda', 0)


@pytest.mark.parametrize("cid", ALL)
def test_golden_case_gpu(cid, golden, dev):
    case = golden.cases[cid]
    got = case_runner.run_case(case, golden, dev)
    if case["op"] == 'Flow.binop' and case["args"]["op"] == 'pow':
        # `vecs ** exponent` is ATen's own pow on the flow's device in the reference as well (flow_class.py:631-678); its GPU
        # kernel is not the CPU's libm pow: 1e-6 of the scale (fp32 tolerance, stated here), masks bit for bit
        _, exp = golden.arrays(case)
        scale = max(float(np.nanmax(np.abs(exp["vecs"]))), 1.0)
        case_runner.check_case(case, golden, got, exact_values=False, rtol=2e-6, atol=1e-6 * scale, max_mask_flips=0)
    elif case["op"] == 'Flow.get_padding' or case["op"].startswith('grad_'):
        # padding lists: exact; gradients: within case_runner.GRAD_RTOL of the gradient scale (forward values and masks
        # recorded with them: bit-exact)
        case_runner.check_case(case, golden, got, exact_values=True)
    elif uses_splat(case):
        _, exp = golden.arrays(case)
        scale = max([float(np.abs(v).max()) for v in exp.values() if v.dtype.kind == 'f' and v.size] + [1.0])
        widths = {int(v.shape[-1]) for v in exp.values() if v.ndim >= 2}
        if min(widths) >= 4:
            case_runner.check_case(case, golden, got, exact_values=True)      # in-order gather path (C <= 3, W >= 4)
        else:                                                                 # the 2 x 2 fixture: two-pass float atomics
            case_runner.check_case(case, golden, got, exact_values=False, rtol=2e-5, atol=2e-5 * scale, max_mask_flips=0)
    else:
        case_runner.check_case(case, golden, got, exact_values=True)


def test_results_stay_on_device(dev):
    import oflibpytorch_amd as ofl
    f = ofl.Flow(torch.randn(2, 2, 33, 47, device=dev) * 3, 't')
    img = torch.rand(2, 3, 33, 47, device=dev)
    w, m = f.apply(img, return_valid_area=True)
    assert w.device == dev and m.device == dev and m.dtype == torch.bool
    out = f.combine_with(ofl.Flow(torch.randn(2, 2, 33, 47, device=dev), 't'), 3)
    assert out.vecs.device == dev and out.mask.device == dev


def test_cpu_tensors_are_staged_through_the_gpu(dev):
    """CPU-resident inputs (the reference's default) still compute on the HIP kernels; results come back on CPU."""
    import oflibpytorch_amd as ofl
    g = torch.Generator().manual_seed(3)
    f = torch.randn(1, 2, 20, 30, generator=g) * 2
    img = torch.rand(1, 3, 20, 30, generator=g)
    w_cpu = ofl.Flow(f, 't').apply(img)
    w_gpu = ofl.Flow(f.to(dev), 't').apply(img.to(dev))
    assert w_cpu.device.type == 'cpu' and torch.equal(w_cpu, w_gpu.cpu())


# ------------------------------------------------------------------------------------------------
# y-sheared staging boxes (flows with a strong dv/dx): shear on == shear off == generic kernel == oracle, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 3, 160, 256), (2, 2, 96, 384), (1, 1, 70, 132), (1, 3, 90, 253), (2, 2, 64, 130)])
@pytest.mark.parametrize("slope", [0.3, -0.8, 2.5, -7.0])
def test_sheared_boxes_agree(shape, slope, dev):
    from oflibpytorch_amd import _native
    from oracle import oracle
    n, c, h, w = shape
    g = torch.Generator().manual_seed(3)
    xs = torch.arange(w, dtype=torch.float32)[None, None, None, :] - w / 2
    ys = torch.arange(h, dtype=torch.float32)[None, None, :, None] - h / 2
    flow = torch.cat([0.15 * ys.expand(n, 1, h, w) + 0.05 * xs, slope * xs.expand(n, 1, h, w) - 0.1 * ys], 1)
    flow = (flow + torch.randn(n, 2, h, w, generator=g) * 0.4).contiguous().to(dev)
    src = (torch.rand(n, c, h, w, generator=g) * 200 - 50).to(dev)
    sm = (torch.rand(n, h, w, generator=g) > 0.1).to(dev)
    fmk = (torch.rand(n, h, w, generator=g) > 0.1).to(dev)
    add = torch.randn(n, c, h, w, generator=g).to(dev)
    for kw in (dict(src_mask=sm, flow_mask=fmk, want_valid=True),
               dict(flow_sign=-1.0, src_mask=sm, want_valid=True, addend=add, a_sign=1.0, g_sign=1.0)):
        outs = []
        for path, shear in ((0, True), (0, False), (1, True)):
            _native.set_warp_path(path)
            _native.set_warp_shear(shear)
            try:
                outs.append(_native.warp_bwd(flow, src, **kw))
            finally:
                _native.set_warp_path(0)
                _native.set_warp_shear(True)
        for other in outs[1:]:
            for a, b in zip(outs[0], other):
                assert (a is None) == (b is None)
                if a is not None:
                    assert torch.equal(a, b), "sheared / plain / generic staging differ for %s" % (kw,)
        f = flow.cpu().numpy() * np.float32(kw.get("flow_sign", 1.0))
        s = np.concatenate([src.cpu().numpy(), sm.cpu().numpy().astype(np.float32)[:, None]], 1)
        gref = oracle.G(f, s)
        exp = gref[:, :c]
        if "addend" in kw:
            exp = np.float32(kw["a_sign"]) * add.cpu().numpy() + np.float32(kw["g_sign"]) * exp
        assert np.array_equal(outs[0][0].cpu().numpy(), exp, equal_nan=True)
        expv = gref[:, c] > np.float32(0.99999)
        if "flow_mask" in kw:
            expv &= fmk.cpu().numpy()
        assert np.array_equal(outs[0][1].cpu().numpy(), expv)


# ------------------------------------------------------------------------------------------------
# the LDS-staged fast path and the generic direct-gather kernel must agree bit for bit, and both with the oracle
# ------------------------------------------------------------------------------------------------
def _smooth(n, h, w, sigma, seed, dev):
    g = torch.Generator().manual_seed(seed)
    lo = torch.randn(n, 2, max(h // 12, 2), max(w // 12, 2), generator=g) * sigma
    return torch.nn.functional.interpolate(lo, size=(h, w), mode='bicubic', align_corners=True).contiguous().to(dev)


@pytest.mark.parametrize("c,stretch,frame", [(1, 1.2, (160, 224)), (2, 1.2, (160, 224)), (3, 1.2, (160, 224)),
                                             (1, 1.6, (160, 224)), (2, 1.6, (160, 224)), (3, 1.6, (160, 224)),
                                             (1, 2.5, (160, 224)), (2, 2.5, (160, 224)), (3, 2.5, (160, 224)),
                                             (1, 6.0, (160, 224)), (2, 6.0, (160, 224)), (3, 6.0, (160, 224)),
                                             (3, 2.5, (150, 218)), (2, 1.6, (147, 221)), (3, 3.5, (100, 330))])   # widths that are not multiples of 4, ragged last tiles
def test_oversize_boxes_staged_in_part_stay_exact(c, stretch, frame, dev):
    """A flow that stretches the sampled region makes a 32 x 16 tile's box larger than the LDS budget (26 KB = 1 663 pixel slots):
    the four-tile column kernel of LARGE launches stages the rows that fit and only the pixels with a tap below them gather from
    global memory (OFL_WARP_CLIP); the two-tile, one-tile and generic kernels do not.  All must agree bit for bit, and with the
    oracle.  stretch 1.2: boxes fit; 1.6 / 2.5: oversize, most rows staged; 6.0: too few rows fit in places (whole-tile fallback).
    The batch is large enough for the launcher to pick the column kernel (>= 6 912 column groups)."""
    from oflibpytorch_amd import _native
    from oracle import oracle
    h, w = frame
    n = 6912 // (((w + 31) // 32) * ((h + 63) // 64)) + 1          # enough column groups (of 4 tiles) for the launcher to pick the column kernel
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    # sample position = pixel - flow: x - u = cx + (x - cx) * stretch, likewise y (plus a smooth wobble, another per image)
    u = -(xs - w / 2) * (stretch - 1.0) * 0.8
    v = -(ys - h / 2) * (stretch - 1.0)
    flow = (torch.stack([u, v])[None] + _smooth(n, h, w, 2.0, 23, torch.device('cpu'))).contiguous().to(dev)
    g = torch.Generator().manual_seed(9)
    src = (torch.rand(n, c, h, w, generator=g) * 100 - 20).to(dev)
    sm = (torch.rand(n, h, w, generator=g) > 0.1).to(dev)
    fmk = (torch.rand(n, h, w, generator=g) > 0.1).to(dev)
    add = torch.randn(n, c, h, w, generator=g).to(dev)
    kws = [dict(src_mask=sm, flow_mask=fmk, want_valid=True), dict()]
    if c == 2:
        # round 5: the fused composition -- the ADD epilogue -- runs on the column kernel too, oversize boxes staged in
        # part: once with the flow itself as the addend (mode 3 proper: the REUSE instantiation re-forms the positions from the
        # flow registers), once with another field
        kws += [dict(src_mask=sm, flow_mask=fmk, want_valid=True, addend=flow, a_sign=1.0, g_sign=1.0),
                dict(flow_mask=fmk, want_valid=True, addend=add, a_sign=-1.0, g_sign=1.0)]
    for kw in kws:
        outs = []
        for path in (0, 1, 3, 4, 6):            # auto (= columns of four here: per-row extents when the launch is lean, W % 4 == 0), generic, two tiles per block, one tile per block, columns of four with the sheared rectangle
            _native.set_warp_path(path)
            try:
                outs.append(_native.warp_bwd(flow, src, **kw))
            finally:
                _native.set_warp_path(0)
        for other in outs[1:]:
            for a, b in zip(outs[0], other):
                assert (a is None) == (b is None)
                if a is not None:
                    assert torch.equal(a, b)
        k = 3                                    # (the oracle on the first images only: it is the checker, not the thing timed)
        s = src[:k].cpu().numpy()
        if kw.get("want_valid"):
            m = sm[:k].cpu().numpy().astype(np.float32) if "src_mask" in kw else np.ones((k, h, w), np.float32)
            s = np.concatenate([s, m[:, None]], 1)
        gref = oracle.G(flow[:k].cpu().numpy(), s)
        exp = gref[:, :c]
        if "addend" in kw:
            exp = np.float32(kw["a_sign"]) * kw["addend"][:k].cpu().numpy() + np.float32(kw["g_sign"]) * exp
        assert np.array_equal(outs[0][0][:k].cpu().numpy(), exp, equal_nan=True)
        if kw.get("want_valid"):
            assert np.array_equal(outs[0][1][:k].cpu().numpy(), (gref[:, c] > 0.99999) & fmk[:k].cpu().numpy())


@pytest.mark.parametrize("kind", ["rotation", "waves", "zoom_in", "steep_rows", "steep_columns", "outward", "blocks"])
@pytest.mark.parametrize("c", [1, 2, 3])
def test_row_tables_on_strongly_curved_flows(kind, c, dev):
    """warp_bwd_rows_kernel (per-row extents of the staged box: every source row a 64 x 16 tile touches has its own first chunk and
    length in a 64-row table about an ESTIMATED origin) against the sheared rectangle (path 6), the generic kernel (path 1) and the
    oracle, on flows that make the rows of a tile differ as much as they can: a rotation (every row another start), waves (curved
    bands), a zoom-in (few short rows), slopes steep enough for rows to fall outside the table and for lanes to span many rows, a
    flow that leaves the frame, and per-block constants (discontinuities: more than 512 chunks -- the extra staging round -- and
    more than the block's budget).  The batch is large enough for the launcher to pick the column kernel."""
    from oflibpytorch_amd import _native
    from oracle import oracle
    h, w = 176, 256
    n = 6912 // (((w + 31) // 32) * ((h + 63) // 64)) + 1
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    cx, cy = w / 2, h / 2
    if kind == "rotation":
        a = 0.45
        u = (xs - cx) - ((xs - cx) * np.cos(a) - (ys - cy) * np.sin(a))
        v = (ys - cy) - ((xs - cx) * np.sin(a) + (ys - cy) * np.cos(a))
    elif kind == "waves":
        u = 9.0 * torch.sin(ys / 7.0) + 4.0 * torch.cos(xs / 5.0)
        v = 14.0 * torch.sin(xs / 9.0) + 3.0 * torch.sin(ys / 4.0)
    elif kind == "zoom_in":
        u = (xs - cx) * 0.7
        v = (ys - cy) * 0.7
    elif kind == "steep_rows":
        u = torch.zeros_like(xs)
        v = (xs - cx) * 1.3 + 6.0 * torch.sin(ys / 5.0)
    elif kind == "steep_columns":
        u = (ys - cy) * 2.2
        v = 5.0 * torch.sin(xs / 6.0)
    elif kind == "outward":
        u = (xs - cx) * 0.2 - 180.0
        v = (ys - cy) * 0.3 + 120.0
    else:
        g0 = torch.Generator().manual_seed(3)
        lo = torch.randn(2, h // 8, w // 8, generator=g0) * 25.0
        u, v = [torch.nn.functional.interpolate(t[None, None], size=(h, w), mode='nearest')[0, 0] for t in lo]
    flow = (torch.stack([u, v])[None] + _smooth(n, h, w, 1.5, 29, torch.device('cpu'))).contiguous().to(dev)
    g = torch.Generator().manual_seed(13)
    src = (torch.rand(n, c, h, w, generator=g) * 100 - 20).to(dev)
    sm = (torch.rand(n, h, w, generator=g) > 0.1).to(dev)
    fmk = (torch.rand(n, h, w, generator=g) > 0.1).to(dev)
    for kw in (dict(src_mask=sm, flow_mask=fmk, want_valid=True), dict(), dict(want_valid=True), dict(flow_sign=-1.0, src_mask=sm, want_valid=True)):
        outs = []
        for path in (0, 6, 1):
            _native.set_warp_path(path)
            try:
                outs.append(_native.warp_bwd(flow, src, **kw))
            finally:
                _native.set_warp_path(0)
        for other in outs[1:]:
            for a_, b_ in zip(outs[0], other):
                assert (a_ is None) == (b_ is None)
                if a_ is not None:
                    assert torch.equal(a_, b_)
        k = 2
        s_ = src[:k].cpu().numpy()
        if kw.get("want_valid"):
            m = sm[:k].cpu().numpy().astype(np.float32) if "src_mask" in kw else np.ones((k, h, w), np.float32)
            s_ = np.concatenate([s_, m[:, None]], 1)
        gref = oracle.G(np.float32(kw.get("flow_sign", 1.0)) * flow[:k].cpu().numpy(), s_)
        assert np.array_equal(outs[0][0][:k].cpu().numpy(), gref[:, :c], equal_nan=True)
        if kw.get("want_valid"):
            fm_ = fmk[:k].cpu().numpy() if "flow_mask" in kw else np.ones((k, h, w), bool)
            assert np.array_equal(outs[0][1][:k].cpu().numpy(), (gref[:, c] > 0.99999) & fm_)


@pytest.mark.parametrize("c", [1, 2, 3])
@pytest.mark.parametrize("kind", ["waves", "blocks"])
def test_row_tables_gradient_wrt_flow(kind, c, dev):
    """The gradient with respect to the flow (ofl_warp_bwd_grad_f32, grad_flow alone) of large launches runs on the row-table kernel (GRAD
    instantiation): == the column kernel on the sheared rectangle (path 6) == the one-pixel-per-lane kernel (path 1), bit for bit."""
    from oflibpytorch_amd import _native
    h, w = 176, 256
    n = 6912 // (((w + 31) // 32) * ((h + 63) // 64)) + 1
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    if kind == "waves":
        u = 9.0 * torch.sin(ys / 7.0) + 4.0 * torch.cos(xs / 5.0)
        v = 14.0 * torch.sin(xs / 9.0) + 3.0 * torch.sin(ys / 4.0)
    else:
        g0 = torch.Generator().manual_seed(3)
        lo = torch.randn(2, h // 8, w // 8, generator=g0) * 25.0
        u, v = [torch.nn.functional.interpolate(t[None, None], size=(h, w), mode='nearest')[0, 0] for t in lo]
    flow = (torch.stack([u, v])[None] + _smooth(n, h, w, 1.5, 41, torch.device('cpu'))).contiguous().to(dev)
    g = torch.Generator().manual_seed(23)
    src = (torch.rand(n, c, h, w, generator=g) * 100 - 20).to(dev)
    go = torch.randn(n, c, h, w, generator=g).to(dev)
    outs = []
    for path in (0, 6, 1):
        _native.set_warp_path(path)
        try:
            outs.append(_native.warp_bwd_grad(flow, src, go, flow_sign=-1.0 if kind == "blocks" else 1.0, g_scale=0.5, want_src=False, want_flow=True)[1])
        finally:
            _native.set_warp_path(0)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    # ... and an INDEPENDENT reference for the first images: torch autograd through the reference's own op sequence (utils.py:541-555,
    # F.grid_sample) on the CPU -- the reference's device, whose fp32 operation order, and so every floor() decision, the HIP kernels
    # restate bit for bit (the gradient wrt positions jumps across cell borders) -- within the tolerance of tests/test_autograd.py
    k = 3
    sign = -1.0 if kind == "blocks" else 1.0
    fl = flow[:k].cpu().clone().requires_grad_(True)
    gy, gx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    field = (torch.stack((gx, gy), dim=-1).float().unsqueeze(0) - sign * fl.permute(0, 2, 3, 1)) * 2
    field = torch.stack((field[..., 0] / (w - 1), field[..., 1] / (h - 1)), dim=-1) - 1
    ref = torch.nn.functional.grid_sample(src[:k].cpu(), field, align_corners=True)
    (gref,) = torch.autograd.grad((ref * (0.5 * go[:k].cpu())).sum(), fl)
    scale = float(gref.abs().max())
    err = float((outs[0][:k].cpu().double() - gref.double()).abs().max())
    assert err <= 2e-4 * max(scale, 1e-6), "grad wrt flow: max |diff| %.3g against a gradient scale of %.3g" % (err, scale)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("kind", ["waves", "blocks"])
def test_row_tables_uint8_images(kind, c, dev):
    """uint8 images warped from and to their bytes (ofl_warp_bwd_u8, round-half-even + clamp) on the row-table kernel of large launches
    (1 or 3 channels, W % 4 == 0): == the two-tile kernel (path 6 / 3) == the generic kernel (path 1), bit for bit, values and valid mask."""
    from oflibpytorch_amd import _native
    h, w = 176, 256
    n = 6912 // (((w + 31) // 32) * ((h + 63) // 64)) + 1
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    if kind == "waves":
        u = 9.0 * torch.sin(ys / 7.0) + 4.0 * torch.cos(xs / 5.0)
        v = 14.0 * torch.sin(xs / 9.0) + 3.0 * torch.sin(ys / 4.0)
    else:
        g0 = torch.Generator().manual_seed(3)
        lo = torch.randn(2, h // 8, w // 8, generator=g0) * 25.0
        u, v = [torch.nn.functional.interpolate(t[None, None], size=(h, w), mode='nearest')[0, 0] for t in lo]
    flow = (torch.stack([u, v])[None] + _smooth(n, h, w, 1.5, 37, torch.device('cpu'))).contiguous().to(dev)
    g = torch.Generator().manual_seed(19)
    src = torch.randint(0, 256, (n, c, h, w), generator=g, dtype=torch.uint8).to(dev)
    sm = (torch.rand(n, h, w, generator=g) > 0.1).to(dev)
    fmk = (torch.rand(n, h, w, generator=g) > 0.1).to(dev)
    for kw in (dict(src_mask=sm, flow_mask=fmk, want_valid=True), dict()):
        outs = []
        for path in (0, 6, 3, 1):
            _native.set_warp_path(path)
            try:
                outs.append(_native.warp_bwd(flow, src, round_mode=_native.ROUND_U8, out_uint8=True, **kw))
                outs[-1] = outs[-1] + _native.warp_bwd(flow, src, **kw)[:2]          # (fp32 out, no rounding: Flow.apply of a uint8 image)
            finally:
                _native.set_warp_path(0)
        assert outs[0][0].dtype == torch.uint8
        for other in outs[1:]:
            for a_, b_ in zip(outs[0], other):
                assert (a_ is None) == (b_ is None)
                if a_ is not None:
                    assert torch.equal(a_, b_)
        # ... and the ORACLE on the first images (the paths above are four kernels of one library: pinned here, not only through each other)
        from oracle import oracle
        k = 3
        s_ = src[:k].cpu().numpy().astype(np.float32)
        if kw.get("want_valid"):
            s_ = np.concatenate([s_, sm[:k].cpu().numpy().astype(np.float32)[:, None]], 1)
        gref = oracle.G(flow[:k].cpu().numpy(), s_)
        exp_u8 = np.clip(np.rint(gref[:, :c]), 0, 255).astype(np.uint8)          # torch.round (half to even) + clamp, flow_class.py:943-946
        assert np.array_equal(outs[0][0][:k].cpu().numpy(), exp_u8)
        assert np.array_equal(outs[0][-2][:k].cpu().numpy(), gref[:, :c])         # (fp32 out, no rounding: the last two of the tuple)
        if kw.get("want_valid"):
            expv = (gref[:, c] > np.float32(0.99999)) & fmk[:k].cpu().numpy()
            assert np.array_equal(outs[0][1][:k].cpu().numpy(), expv) and np.array_equal(outs[0][-1][:k].cpu().numpy(), expv)


@pytest.mark.parametrize("kind", ["waves", "steep_rows", "blocks", "outward"])
@pytest.mark.parametrize("c,valid", [(8, False), (7, True), (9, False)])
def test_channel_loop_with_row_tables(kind, c, valid, dev):
    """The channel-loop kernel of LARGE many-channel warps (64 x 16 tiles, >= 13 824 tiles) forms its per-tile invariants -- chunk map,
    tap addresses -- from per-row extents (warp_bwd_lds_chan_kernel<.., ROWS>); against the same kernel on the sheared rectangle
    (path 6), separate launches of 3 channels (path 5) and the generic kernel (path 1), bit for bit, on flows that curve, leave the
    table, leave the frame or jump (rows beyond the block's chunk budget: those pixels take the global fix-up)."""
    from oflibpytorch_amd import _native
    h, w = 176, 256
    n = 2 * 6912 // (((w + 31) // 32) * ((h + 15) // 16)) + 2
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
    cx, cy = w / 2, h / 2
    if kind == "waves":
        u = 9.0 * torch.sin(ys / 7.0) + 4.0 * torch.cos(xs / 5.0)
        v = 14.0 * torch.sin(xs / 9.0) + 3.0 * torch.sin(ys / 4.0)
    elif kind == "steep_rows":
        u = torch.zeros_like(xs)
        v = (xs - cx) * 1.3 + 6.0 * torch.sin(ys / 5.0)
    elif kind == "outward":
        u = (xs - cx) * 0.2 - 180.0
        v = (ys - cy) * 0.3 + 120.0
    else:
        g0 = torch.Generator().manual_seed(3)
        lo = torch.randn(2, h // 8, w // 8, generator=g0) * 25.0
        u, v = [torch.nn.functional.interpolate(t[None, None], size=(h, w), mode='nearest')[0, 0] for t in lo]
    flow = (torch.stack([u, v])[None] + _smooth(n, h, w, 1.5, 31, torch.device('cpu'))).contiguous().to(dev)
    g = torch.Generator().manual_seed(17)
    src = (torch.rand(n, c, h, w, generator=g) * 100 - 20).to(dev)
    sm = (torch.rand(n, h, w, generator=g) > 0.1).to(dev)
    fmk = (torch.rand(n, h, w, generator=g) > 0.1).to(dev)
    kw = dict(src_mask=sm, flow_mask=fmk, want_valid=True) if valid else dict()
    outs = []
    for path in (0, 6, 5, 1):
        _native.set_warp_path(path)
        try:
            outs.append(_native.warp_bwd(flow, src, **kw))
        finally:
            _native.set_warp_path(0)
    for other in outs[1:]:
        for a_, b_ in zip(outs[0], other):
            assert (a_ is None) == (b_ is None)
            if a_ is not None:
                assert torch.equal(a_, b_)
    # ... and the ORACLE on the first images
    from oracle import oracle
    k = 2
    s_ = src[:k].cpu().numpy()
    if valid:
        s_ = np.concatenate([s_, sm[:k].cpu().numpy().astype(np.float32)[:, None]], 1)
    gref = oracle.G(flow[:k].cpu().numpy(), s_)
    assert np.array_equal(outs[0][0][:k].cpu().numpy(), gref[:, :c], equal_nan=True)
    if valid:
        assert np.array_equal(outs[0][1][:k].cpu().numpy(), (gref[:, c] > np.float32(0.99999)) & fmk[:k].cpu().numpy())


@pytest.mark.parametrize("shape", [(2, 3, 64, 96), (1, 2, 37, 52), (2, 1, 16, 4), (1, 3, 2, 8), (3, 2, 130, 260),
                                   (2, 3, 37, 50), (2, 2, 33, 47), (1, 1, 19, 6), (1, 3, 70, 129), (2, 2, 40, 5),    # widths that are not multiples of 4
                                   (2, 4, 40, 64), (1, 7, 33, 45), (2, 6, 20, 36),                               # more than 3 channels: the channel-loop kernel (W % 4 == 0) / groups of 3
                                   (1, 5, 64, 96), (2, 9, 70, 128), (1, 16, 130, 260), (1, 64, 48, 64)])
@pytest.mark.parametrize("sigma", [0.0005, 3.0, 40.0])
def test_lds_and_generic_paths_agree(shape, sigma, dev):
    import sys
    from oflibpytorch_amd import _native
    from oracle import oracle
    n, c, h, w = shape
    flow = _smooth(n, h, w, sigma, 11, dev)
    if sigma > 10:
        flow[0, :, : h // 2] *= 20            # huge displacements: bounding boxes that cannot fit LDS -> per-tile fallback
    g = torch.Generator().manual_seed(5)
    src = (torch.rand(n, c, h, w, generator=g) * 200 - 50).to(dev)
    sm = (torch.rand(n, h, w, generator=g) > 0.1).to(dev)
    fmk = (torch.rand(n, h, w, generator=g) > 0.1).to(dev)
    add = torch.randn(n, c, h, w, generator=g).to(dev)
    for kw in (dict(), dict(src_mask=sm, flow_mask=fmk, want_valid=True), dict(want_valid=True),
               dict(flow_sign=-1.0, src_mask=sm, want_valid=True, addend=add, a_sign=1.0, g_sign=-1.0),
               dict(round_mode=2), dict(flow_mask=fmk, want_valid=True, want_flags=True, want_src_flags=(c == 2))):
        outs = []
        for path in (0, 1, 3, 4, 5, 6, 7):      # auto (lean launches: row tables, 1 or 2 tiles per block at these sizes), generic, staged two tiles per block, staged one tile per block, > 3 channels as launches of 3, the sheared rectangle, four-tile columns with row tables whatever the size
            if path == 5 and c <= 3:
                continue
            _native.set_warp_path(path)
            try:
                outs.append(_native.warp_bwd(flow, src, **kw))
            finally:
                _native.set_warp_path(0)
        for other in outs[1:]:
            for a, b in zip(outs[0], other):
                assert (a is None) == (b is None)
                if a is not None:
                    assert torch.equal(a, b), "the warp kernels differ for %s" % (kw,)
        # and against the oracle (values bit-exact, masks bit-exact)
        f = flow.cpu().numpy() * np.float32(kw.get("flow_sign", 1.0))
        s = src.cpu().numpy()
        if kw.get("want_valid"):
            m = sm.cpu().numpy().astype(np.float32) if "src_mask" in kw else np.ones((n, h, w), np.float32)
            s = np.concatenate([s, m[:, None]], 1)
        gref = oracle.G(f, s)
        exp = gref[:, :c]
        if "addend" in kw:
            exp = np.float32(kw["a_sign"]) * add.cpu().numpy() + np.float32(kw["g_sign"]) * exp
        if kw.get("round_mode"):
            exp = np.clip(np.rint(exp), 0, 255).astype(np.float32)
        assert np.array_equal(outs[0][0].cpu().numpy(), exp, equal_nan=True)
        if kw.get("want_valid"):
            v = oracle.theta(gref[:, c])
            if "flow_mask" in kw:
                v = v & fmk.cpu().numpy()
            assert np.array_equal(outs[0][1].cpu().numpy(), v)
        if kw.get("want_flags"):
            assert np.array_equal(outs[0][2].cpu().numpy(), oracle.flow_flags(flow.cpu().numpy(), fmk.cpu().numpy()))
            if c == 2:
                assert np.array_equal(outs[0][3].cpu().numpy(), oracle.flow_flags(src.cpu().numpy(), None))


def test_exact_division_corner_cases(dev):
    """Operands the reciprocal division cannot take (huge, and tiny non-zero in column / row 0) go through the IEEE divide."""
    from oflibpytorch_amd import _native
    from oracle import oracle
    h, w = 16, 32
    flow = torch.zeros(1, 2, h, w)
    flow[0, 0, :, 0] = 1e-30          # x - u tiny but non-zero in column 0
    flow[0, 1, 0, :] = -3e-33         # y - v tiny in row 0
    flow[0, 0, 5, 7] = 3e37           # overflow when doubled
    flow[0, 1, 9, 3] = -2.5e31
    flow[0, 0, 3, 3] = 1.7
    src = torch.rand(1, 3, h, w) * 10
    for path in (0, 1):
        _native.set_warp_path(path)
        try:
            out, valid, _, _ = _native.warp_bwd(flow.to(dev), src.to(dev), want_valid=True)
        finally:
            _native.set_warp_path(0)
        ref = oracle.G(flow.numpy(), np.concatenate([src.numpy(), np.ones((1, 1, h, w), np.float32)], 1))
        assert np.array_equal(out.cpu().numpy(), ref[:, :3], equal_nan=True)
        assert np.array_equal(valid.cpu().numpy(), oracle.theta(ref[:, 3]))


# ------------------------------------------------------------------------------------------------
# forward splat: the fused tiled kernel vs the two-pass atomics path vs the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 64, 96), (1, 2, 37, 52), (2, 1, 16, 4), (3, 3, 130, 260), (2, 3, 45, 97), (1, 2, 30, 66), (2, 5, 40, 52)])
@pytest.mark.parametrize("sigma", [0.0, 3.0, 60.0])
def test_tiled_splat_matches_two_pass_and_oracle(shape, sigma, dev):
    from oflibpytorch_amd import _native
    from oracle import oracle
    n, c, h, w = shape
    flow = _smooth(n, h, w, max(sigma, 1.0), 21, dev)
    if sigma == 0.0:
        flow = flow * 0 + 2e-4                      # everything below the zero-flow threshold: pure un-occlude fill
    flow[0, :, h // 4: h // 2, w // 4: w // 2] = 0   # zero-flow block (occlusion rule)
    if sigma > 10:
        flow[-1] *= 6                               # rough: candidate lists overflow -> in-call atomics fallback
    g = torch.Generator().manual_seed(9)
    data = (torch.rand(n, c, h, w, generator=g) * 100 - 20).to(dev)
    wm = (torch.rand(n, h, w, generator=g) > 0.15).to(dev)
    ca = (torch.rand(n, h, w, generator=g) > 0.15).to(dev)
    for kw in (dict(weight_mask=wm, chan_mask_a=ca, chan_mask_b=wm, want_valid=True, want_density=True, want_warped=True),
               dict(want_warped=True), dict(weight_mask=wm, occlude=False, want_density=True),
               dict(flow_sign=-1.0, data_sign=-1.0, chan_mask_a=ca, weight_mask=wm, want_mask_chan=True)):
        outs = []
        for path in (0, 1):
            _native.set_splat_path(path)
            try:
                outs.append(_native.splat_fwd(flow, data, **kw))
            finally:
                _native.set_splat_path(0)
        scale = 120.0
        for a, b in zip(*outs):
            assert (a is None) == (b is None)
            if a is None:
                continue
            if a.dtype == torch.bool:
                assert torch.equal(a, b), "masks differ between tiled and two-pass splat for %s" % (kw,)
            else:
                np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=3e-5, atol=3e-5 * scale)
        # oracle
        f = flow.cpu().numpy() * np.float32(kw.get("flow_sign", 1.0))
        d = data.cpu().numpy() * np.float32(kw.get("data_sign", 1.0))
        mc = np.ones((n, h, w), bool)
        for key in ("chan_mask_a", "chan_mask_b"):
            if key in kw:
                mc &= kw[key].cpu().numpy()
        dd = np.concatenate([d, mc[:, None].astype(np.float32)], 1)
        m = kw["weight_mask"].cpu().numpy() if "weight_mask" in kw else None
        ref, rwarped, rden = oracle.apply_s_flow(f, dd, m, kw.get("occlude", True), return_density=True)
        np.testing.assert_allclose(outs[0][0].cpu().numpy(), ref[:, :c], rtol=3e-5, atol=3e-5 * scale)
        if kw.get("want_valid"):
            assert np.array_equal(outs[0][1].cpu().numpy(), oracle.theta(ref[:, c]))
        if kw.get("want_mask_chan"):
            np.testing.assert_allclose(outs[0][1].cpu().numpy(), ref[:, c], rtol=3e-5, atol=3e-5)
            assert np.array_equal(outs[0][1].cpu().numpy() == 1, ref[:, c] == 1)
        if kw.get("want_density"):
            np.testing.assert_allclose(outs[0][2].cpu().numpy(), rden, rtol=3e-5, atol=1e-5)
        if kw.get("want_warped"):
            assert np.array_equal(outs[0][3].cpu().numpy(), rwarped)


@pytest.mark.parametrize("shape", [(2, 3, 64, 96), (1, 2, 70, 132), (2, 1, 48, 64), (1, 3, 130, 260),
                                   (2, 3, 37, 50), (1, 2, 33, 47), (2, 1, 40, 65), (1, 3, 70, 129), (1, 3, 20, 5),    # any width
                                   (2, 4, 40, 64), (1, 7, 33, 45)])                                                # > 3 channels: groups of 3
@pytest.mark.parametrize("sigma", [0.7, 1.5])
def test_exact_splat_is_bit_identical_to_the_oracle(shape, sigma, dev):
    """The exact tile path sums each destination pixel's contributions per corner class in raster order of the sources,
    then ((c0 + c1) + c2) + c3: the reference's order (utils.py:1133-1143).  No tolerance."""
    from oflibpytorch_amd import _native
    from oracle import oracle
    n, c, h, w = shape
    flow = _smooth(n, h, w, sigma, 33, dev)
    flow[0, :, h // 4: h // 2, w // 4: w // 2] = 0
    g = torch.Generator().manual_seed(10)
    data = (torch.rand(n, c, h, w, generator=g) * 100 - 20).to(dev)
    wm = (torch.rand(n, h, w, generator=g) > 0.15).to(dev)
    ca = (torch.rand(n, h, w, generator=g) > 0.15).to(dev)
    try:
        for kw in (dict(weight_mask=wm, chan_mask_a=ca, want_mask_chan=True, want_density=True, want_warped=True),
                   dict(want_density=True), dict(flow_sign=-1.0, data_sign=-1.0, weight_mask=wm, occlude=False, want_density=True)):
            for rep in range(2):                       # and run to run
                out = _native.splat_fwd(flow, data, **kw)
                f = flow.cpu().numpy() * np.float32(kw.get("flow_sign", 1.0))
                d = data.cpu().numpy() * np.float32(kw.get("data_sign", 1.0))
                mc = kw["chan_mask_a"].cpu().numpy() if "chan_mask_a" in kw else np.ones((n, h, w), bool)
                dd = np.concatenate([d, mc[:, None].astype(np.float32)], 1)
                m = kw["weight_mask"].cpu().numpy() if "weight_mask" in kw else None
                ref, rwarped, rden = oracle.apply_s_flow(f, dd, m, kw.get("occlude", True), return_density=True)
                assert np.array_equal(out[0].cpu().numpy(), ref[:, :c]), "values differ from the oracle (%s)" % (kw,)
                assert np.array_equal(out[2].cpu().numpy(), rden)
                if kw.get("want_mask_chan"):
                    assert np.array_equal(out[1].cpu().numpy(), ref[:, c])
                if kw.get("want_warped"):
                    assert np.array_equal(out[3].cpu().numpy(), rwarped)
    finally:
        pass


@pytest.mark.parametrize("patch", [(12, 0.5), (16, 0.3), (20, 0.2), (24, 0.16), (22, 0.15)])
def test_compressing_flows_stay_exact(patch, dev):
    """Patches of the image that the flow shrinks put many source pixels into one unit cell of the destination grid (here 4
    to ~50 per cell, beyond the four sorted slots of a cell): their lists are put in raster order -- up to 12 records by one
    lane, 13 to 64 by a whole wave (round 4: sp_order_big_cell) -- and still summed in the reference's order: bit-identical
    values, no tile leaves the exact path."""
    from oflibpytorch_amd import _native
    from oracle import oracle
    _native.collect_splat_stats = True
    n, c, h, w = 2, 3, 96, 160
    size, sc = patch
    flow = _smooth(n, h, w, 0.4, 5, torch.device('cpu'))
    for (y0, x0) in ((10, 20), (50, 100), (70, 30)):
        xs = torch.arange(size, dtype=torch.float32).view(1, 1, size) - size / 2 + 0.3
        ys = torch.arange(size, dtype=torch.float32).view(1, size, 1) - size / 2 + 0.7
        flow[:, 0, y0:y0 + size, x0:x0 + size] += (sc - 1.0) * xs
        flow[:, 1, y0:y0 + size, x0:x0 + size] += (sc - 1.0) * ys
    flow = flow.contiguous().to(dev)
    g = torch.Generator().manual_seed(3)
    data = (torch.rand(n, c, h, w, generator=g) * 100 - 20).to(dev)
    wm = (torch.rand(n, h, w, generator=g) > 0.1).to(dev)
    ca = (torch.rand(n, h, w, generator=g) > 0.1).to(dev)
    kw = dict(weight_mask=wm, chan_mask_a=ca, want_mask_chan=True, want_density=True, want_warped=True)
    out = _native.splat_fwd(flow, data, **kw)
    assert _native._last_splat_stats.cpu().tolist()[:2] == [0, 0]
    dd = np.concatenate([data.cpu().numpy(), ca.cpu().numpy()[:, None].astype(np.float32)], 1)
    ref, rwarped, rden = oracle.apply_s_flow(flow.cpu().numpy(), dd, wm.cpu().numpy(), True, return_density=True)
    assert rden.max() > 3.5                                   # the case does exercise long cell lists
    if sc < 0.18:
        assert rden.max() > 20.0                              # ... and the wave-ordered ones (more than 12 records in a cell)
    assert np.array_equal(out[0].cpu().numpy(), ref[:, :c])
    assert np.array_equal(out[1].cpu().numpy(), ref[:, c])
    assert np.array_equal(out[2].cpu().numpy(), rden)
    assert np.array_equal(out[3].cpu().numpy(), rwarped)


@pytest.mark.parametrize("c,with_holes", [(3, True), (2, False), (2, True)])
def test_overflowing_tiles_are_summed_in_planned_bands(c, with_holes, dev):
    """Round 6: a tile whose records overflow the LDS is cut into bands of rows by the FIRST launch, from the exact record counts of its
    cell rows, and the second launch sums a band per block.  Here the frame is squeezed horizontally by a factor that grows from row to
    row (1.2 at the top of every 16-row tile to 5.5 at its bottom): 3 000-odd records per tile in the strip, most of them in its lower
    rows -- bands of very different heights.  Every band fits (no fold), every value is the reference's bit for bit; with holes in the
    mask channel some tiles sum it and their neighbours leave it out (the all-valid shortcut of phase C)."""
    from oflibpytorch_amd import _native
    from oracle import oracle
    _native.collect_splat_stats = True
    n, h, w = 2, 96, 640
    xs = torch.arange(w, dtype=torch.float32).view(1, w)
    ys = torch.arange(h, dtype=torch.float32).view(h, 1)
    squeeze = 1.2 + 4.3 * ((ys % 16) / 15.0)                            # per row
    x0, d0 = 24.0, 256.0
    inside = (xs >= x0) & (xs < x0 + 560.0)
    dest = torch.where(inside, d0 + (xs - x0) / squeeze, xs.expand(h, w))
    flow = torch.zeros(n, 2, h, w)
    flow[:, 0] = (dest - xs).view(1, h, w)
    flow = (flow + _smooth(n, h, w, 0.02, 7, torch.device('cpu'))).contiguous().to(dev)
    g = torch.Generator().manual_seed(12)
    data = (torch.rand(n, c, h, w, generator=g) * 100 - 20).to(dev)
    wm = inside.expand(h, w).view(1, h, w).expand(n, h, w).contiguous().to(dev)
    ca = torch.ones(n, h, w, dtype=torch.bool)
    if with_holes:
        ca[:, 20:40, 100:300] = False
        ca[1, 70:75] = False
    ca = ca.to(dev)
    kw = dict(weight_mask=wm, chan_mask_a=ca, want_mask_chan=True, want_density=True, want_warped=True, occlude=False)
    outs = [_native.splat_fwd(flow, data, **kw) for _ in range(2)]
    st = _native._last_splat_stats.cpu().tolist()
    assert st[0] == 0 and st[1] == 0 and st[3] >= 8, st                 # no fallback image, no fold, band units in the second launch
    dd = np.concatenate([data.cpu().numpy(), ca.cpu().numpy()[:, None].astype(np.float32)], 1)
    ref, rwarped, rden = oracle.apply_s_flow(flow.cpu().numpy(), dd, wm.cpu().numpy(), False, return_density=True)
    assert rden.max() > 5.0
    for out in outs:
        assert np.array_equal(out[0].cpu().numpy(), ref[:, :c])
        assert np.array_equal(out[1].cpu().numpy(), ref[:, c])
        assert np.array_equal(out[2].cpu().numpy(), rden)
        assert np.array_equal(out[3].cpu().numpy(), rwarped)


@pytest.mark.parametrize("c,squeeze,cols", [(3, 7.2, 40), (2, 9.2, 31), (3, 5.3, 52), (2, 7.6, 38)])
def test_many_medium_cells_in_one_tile_stay_exact(c, squeeze, cols, dev):
    """A strip of the frame squeezed horizontally: `cols` destination columns in which EVERY cell holds `squeeze` records, and
    nothing else contributes (the weight mask is off outside the strip) -- as many cells per band as the record store allows that
    are too long for one lane's sorting network (more than six records with three data channels, more than eight with two) and go
    to the waves' queue, or just short enough for the network.  The queue holds one entry per such cell (fuzz seed 31 found it
    sized for cells beyond 12 records when the threshold had moved to 6): bit-identical to the oracle, no tile leaves the exact path."""
    from oflibpytorch_amd import _native
    from oracle import oracle
    _native.collect_splat_stats = True
    n, h, w = 2, 64, 512
    xs = torch.arange(w, dtype=torch.float32)
    x0, d0, wide = 40.0, 256.0, cols * squeeze                        # the strip's destination columns start on a tile boundary
    inside = (xs >= x0) & (xs < x0 + wide)
    dest = torch.where(inside, d0 + (xs - x0) / squeeze, xs)
    flow = torch.zeros(n, 2, h, w)
    flow[:, 0] = (dest - xs).view(1, 1, w)
    flow = (flow + _smooth(n, h, w, 0.02, 3, torch.device('cpu'))).contiguous().to(dev)
    g = torch.Generator().manual_seed(11)
    data = (torch.rand(n, c, h, w, generator=g) * 100 - 20).to(dev)
    wm = inside.view(1, 1, w).expand(n, h, w).contiguous().to(dev)
    out = _native.splat_fwd(flow, data, weight_mask=wm, want_density=True, want_warped=True, occlude=False)
    assert _native._last_splat_stats.cpu().tolist()[:2] == [0, 0]
    ref, rwarped, rden = oracle.apply_s_flow(flow.cpu().numpy(), data.cpu().numpy(), wm.cpu().numpy(), False, return_density=True)
    assert (rden > squeeze - 1.5).sum() > 0.8 * n * h * cols   # the strip: long cells in every row
    assert np.array_equal(out[0].cpu().numpy(), ref[:, :c])
    assert np.array_equal(out[2].cpu().numpy(), rden)
    assert np.array_equal(out[3].cpu().numpy(), rwarped)


@pytest.mark.parametrize("shape", [(3, 70, 132), (2, 37, 50), (1, 9, 3), (2, 64, 96)])
def test_flows_stored_in_fp16_are_converted_and_validated_in_one_pass(shape, dev):
    """ofl_flow_from_f16 (Flow(fp16 tensor) on a HIP device): the fp32 vectors are exactly `.float()`, the flag words those
    of ofl_flow_flags_f32 over them; a NaN still raises the reference's ValueError; odd sizes take the torch conversion."""
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _native
    n, h, w = shape
    v16 = _smooth(n, h, w, 2.0, 31, dev).half()
    v16[0, :, : h // 2] = 0
    g = torch.Generator().manual_seed(3)
    m = (torch.rand(n, h, w, generator=g) > 0.3).to(dev)
    got, flags = _native.flow_from_half(v16, m)
    assert got.dtype == torch.float32 and torch.equal(got, v16.float())
    assert flags.cpu().tolist() == _native.flow_flags(v16.float(), m).cpu().tolist()
    f = ofl.Flow(v16, 't', m)
    assert f.vecs.dtype == torch.float32 and torch.equal(f.vecs, v16.float())
    assert f._flags() == [int(x) for x in _native.flow_flags(v16.float(), m).cpu().tolist()]
    bad = v16.clone()
    bad[n - 1, 1, h - 1, w - 1] = float('nan')
    with pytest.raises(ValueError):
        ofl.Flow(bad, 't', m)


def test_folding_flows_choose_their_path_deterministically(dev):
    """A rough flow (folds: long lists per destination tile, tiles in bands, some on the float-atomics fallback): which
    path a tile takes depends on COUNTS only (records wanted, list lengths), never on the order the atomics landed in --
    the statistics, the masks and every tile that stayed on the exact path are identical from run to run."""
    from oflibpytorch_amd import _native
    _native.collect_splat_stats = True
    n, c, h, w = 2, 3, 540, 960
    import bench
    flow = bench.smooth_flow(n, h, w, 12.0, 3, dev)          # folds
    g = torch.Generator().manual_seed(2)
    data = (torch.rand(n, c, h, w, generator=g) * 100).to(dev)
    stats, outs = [], []
    for rep in range(6):
        outs.append(_native.splat_fwd(flow, data, want_density=True, occlude=False))
        st = _native._last_splat_stats.cpu().tolist()
        assert st[0] == 0
        stats.append(st[:3])
    assert all(s_ == stats[0] for s_ in stats), stats
    for o in outs[1:]:
        assert torch.equal(o[2] > 0, outs[0][2] > 0)
        if stats[0][1] == 0:
            assert torch.equal(o[0], outs[0][0]) and torch.equal(o[2], outs[0][2])


def test_queue_capacity_exceeded_takes_the_two_pass_path(dev):
    """A flow that shrinks the whole frame five-fold sends ~25 source pixels per destination pixel to the tiles in the
    middle: more source subtiles than a destination tile's list holds (128).  The image is flagged on the device and the
    two-pass path redoes it inside the same call: masks bit-exact, values within the stated tolerance."""
    from oflibpytorch_amd import _native
    from oracle import oracle
    _native.collect_splat_stats = True
    n, c, h, w = 1, 2, 256, 384
    xs = torch.arange(w, dtype=torch.float32).view(1, 1, 1, w)
    ys = torch.arange(h, dtype=torch.float32).view(1, 1, h, 1)
    flow = torch.cat([(-0.8 * (xs - 190.3)).expand(n, 1, h, w), (-0.8 * (ys - 120.7)).expand(n, 1, h, w)], 1).contiguous().to(dev)
    g = torch.Generator().manual_seed(8)
    data = (torch.rand(n, c, h, w, generator=g) * 10).to(dev)
    wm = (torch.rand(n, h, w, generator=g) > 0.1).to(dev)
    out = _native.splat_fwd(flow, data, weight_mask=wm, chan_mask_a=wm, want_valid=True, want_density=True, want_warped=True)
    assert _native._last_splat_stats.cpu().tolist()[0] == 1
    dd = np.concatenate([data.cpu().numpy(), wm.cpu().numpy()[:, None].astype(np.float32)], 1)
    ref, rwarped, rden = oracle.apply_s_flow(flow.cpu().numpy(), dd, wm.cpu().numpy(), True, return_density=True)
    assert np.array_equal(out[3].cpu().numpy(), rwarped)
    assert np.array_equal(out[1].cpu().numpy(), oracle.theta(ref[:, c]))
    np.testing.assert_allclose(out[0].cpu().numpy(), ref[:, :c], rtol=3e-5, atol=3e-4)
    np.testing.assert_allclose(out[2].cpu().numpy(), rden, rtol=3e-5, atol=1e-4)


@pytest.mark.parametrize("slots", [1, 2, 0])
def test_fallback_accumulator_is_bounded_and_served_in_rounds(slots, dev):
    """VERDICT r2 (footprint): the two-pass fallback accumulator of the gather splat no longer grows with the batch -- it holds
    `ofl_splat_tiled_fallback_images` images (the pass, capped at 1 GiB) and flagged images beyond that are served in rounds.
    Five images, three of them (0, 2, 4) shrinking the frame ten-fold (their lists overflow: two-pass path), with 1, 2 and
    'automatic' accumulator slots: the same masks bit for bit, values within the two-pass tolerance against the oracle, the
    in-order images (1, 3) bit-exact and identical whatever the slot count."""
    from oflibpytorch_amd import _native
    from oracle import oracle
    _native.collect_splat_stats = True
    n, c, h, w = 5, 2, 256, 384
    xs = torch.arange(w, dtype=torch.float32).view(1, 1, 1, w)
    ys = torch.arange(h, dtype=torch.float32).view(1, 1, h, 1)
    shrink = torch.cat([(-0.9 * (xs - 190.3)).expand(1, 1, h, w), (-0.9 * (ys - 120.7)).expand(1, 1, h, w)], 1)   # ten-fold: every tile the frame lands on lists several times its capacity, whatever the tile width of the build
    smooth = _smooth(2, h, w, 3.0, 31, torch.device('cpu'))
    flow = torch.cat([shrink, smooth[:1], shrink * 0.97, smooth[1:], shrink * 1.02], 0).contiguous().to(dev)
    g = torch.Generator().manual_seed(18)
    data = (torch.rand(n, c, h, w, generator=g) * 10).to(dev)
    wm = (torch.rand(n, h, w, generator=g) > 0.1).to(dev)
    lib = _native.load_library()
    assert lib.ofl_splat_tiled_fallback_images(64, 5, 1080, 1920) * 5 * 1080 * 1920 * 4 <= (1 << 30)     # B = 64 C = 3 + mask: 1 GiB, not 2.65 GB
    assert lib.ofl_splat_tiled_fallback_images(2, 5, 1080, 1920) == 2
    try:
        _native.set_splat_fallback_slots(slots)
        assert lib.ofl_splat_tiled_fallback_images(n, 1 + c + 1, h, w) == (slots if slots else n)
        out = _native.splat_fwd(flow, data, weight_mask=wm, chan_mask_a=wm, want_valid=True, want_density=True, want_warped=True)
        st = _native._last_splat_stats.cpu().tolist()
    finally:
        _native.set_splat_fallback_slots(0)
    assert st[0] == 1 and st[2] == 3                              # three images on the two-pass path
    dd = np.concatenate([data.cpu().numpy(), wm.cpu().numpy()[:, None].astype(np.float32)], 1)
    ref, rwarped, rden = oracle.apply_s_flow(flow.cpu().numpy(), dd, wm.cpu().numpy(), True, return_density=True)
    assert np.array_equal(out[3].cpu().numpy(), rwarped)
    assert np.array_equal(out[1].cpu().numpy(), oracle.theta(ref[:, c]))
    np.testing.assert_allclose(out[0].cpu().numpy(), ref[:, :c], rtol=3e-5, atol=3e-4)
    np.testing.assert_allclose(out[2].cpu().numpy(), rden, rtol=3e-5, atol=1e-4)
    for i in (1, 3):                                              # the in-order images: the reference's sums, bit for bit
        assert np.array_equal(out[0][i].cpu().numpy(), ref[i, :c]) and np.array_equal(out[2][i].cpu().numpy(), rden[i])


def test_a_fold_beyond_the_list_limit_falls_back_per_tile(dev):
    """Every source pixel of a 64-row band ends in ONE row of cells (> 64 per cell): those tiles take the float-atomics
    fallback (counted), masks stay bit-exact, values within the stated tolerance; the choice is the same in every run."""
    from oflibpytorch_amd import _native
    from oracle import oracle
    _native.collect_splat_stats = True
    n, c, h, w = 1, 2, 128, 96
    ys = torch.arange(h, dtype=torch.float32).view(1, 1, h, 1)
    v = torch.where((ys >= 32) & (ys < 112), 60.4 - ys, torch.zeros_like(ys)).expand(n, 1, h, w)
    flow = torch.cat([torch.full((n, 1, h, w), 0.3), v], 1).contiguous().to(dev)
    g = torch.Generator().manual_seed(4)
    data = (torch.rand(n, c, h, w, generator=g) * 10).to(dev)
    outs, stats = [], []
    for rep in range(2):
        outs.append(_native.splat_fwd(flow, data, want_density=True, want_warped=True, occlude=False))
        stats.append(_native._last_splat_stats.cpu().tolist()[:2])
    assert stats[0] == stats[1] and stats[0][0] == 0 and stats[0][1] > 0
    ref, rwarped, rden = oracle.apply_s_flow(flow.cpu().numpy(), data.cpu().numpy(), None, False, return_density=True)
    assert np.array_equal(outs[0][3].cpu().numpy(), rwarped)
    np.testing.assert_allclose(outs[0][0].cpu().numpy(), ref, rtol=2e-5, atol=2e-4)
    np.testing.assert_allclose(outs[0][2].cpu().numpy(), rden, rtol=2e-5, atol=1e-5)


@pytest.mark.parametrize("shape", [(3, 70, 132), (2, 33, 47), (1, 16, 4), (2, 9, 3)])
@pytest.mark.parametrize("kind", ["sum", "cancel", "tiny", "generic"])
def test_warp_output_flags_equal_a_flag_pass_over_the_output(shape, kind, dev):
    """ofl_warp_bwd_f32's dst_flags (the flag word of a + g * G read as a flow under `valid`) against ofl_flow_flags_f32
    over the stored output: staged kernel, generic kernel (narrow frames / forced), cancelling and sub-threshold sums."""
    from oflibpytorch_amd import _native
    n, h, w = shape
    flow = _smooth(n, h, w, 1.5, 9, dev)
    src = _smooth(n, h, w, 3.0, 10, dev)
    g = torch.Generator().manual_seed(6)
    sm = (torch.rand(n, h, w, generator=g) > 0.2).to(dev)
    fm = (torch.rand(n, h, w, generator=g) > 0.2).to(dev)
    kw = dict(src_mask=sm, flow_mask=fm, want_valid=True, want_dst_flags=True)
    if kind == "sum":
        kw.update(addend=flow)
    elif kind == "cancel":                                   # src - G(0, src): zero wherever the zero-flow gather is an exact identity
        src = flow
        flow = torch.zeros_like(flow)
        kw.update(addend=src, a_sign=1.0, g_sign=-1.0)
    elif kind == "tiny":
        src = src * 1e-5
    try:
        if kind == "generic":
            _native.set_warp_path(1)
        out = _native.warp_bwd(flow, src, **kw)
    finally:
        _native.set_warp_path(0)
    assert out[4].cpu().tolist() == _native.flow_flags(out[0], out[1]).cpu().tolist()


@pytest.mark.parametrize("kind", ["smooth", "zero", "tiny", "masked_out", "rough_two_pass", "general_path"])
def test_splat_output_flags_equal_a_flag_pass_over_the_output(kind, dev):
    """The gather splat returns the flag word of its OUTPUT (read as a flow under its valid mask) as a by-product; it
    must equal what ofl_flow_flags_f32 computes from the stored tensors -- on the exact path, on the per-tile and
    launch-level fallbacks and on the general two-pass path."""
    from oflibpytorch_amd import _native
    n, h, w = 3, 70, 132
    flow = _smooth(n, h, w, 1.5, 9, dev)
    data = _smooth(n, h, w, 3.0, 10, dev)
    g = torch.Generator().manual_seed(5)
    wm = (torch.rand(n, h, w, generator=g) > 0.2).to(dev)
    ca = (torch.rand(n, h, w, generator=g) > 0.2).to(dev)
    if kind == "zero":
        data = torch.zeros_like(data)
    elif kind == "tiny":
        data = data * 1e-5                                   # non-zero, but below the 1e-3 threshold
    elif kind == "masked_out":
        data[1] = 0
        ca[0] = False                                        # nothing valid in image 0, all-zero vectors in image 1
    elif kind == "rough_two_pass":
        flow = _smooth(n, h, w, 400.0, 9, dev)               # source tiles spread too wide: launch-level fallback
    try:
        if kind == "general_path":
            _native.set_splat_path(1)
        out = _native.splat_fwd(flow, data, weight_mask=wm, chan_mask_a=ca, want_valid=True, want_dst_flags=True)
        _native.set_splat_pass_images(1)                     # ... and with one image per pass (flag words per pass)
        out1 = _native.splat_fwd(flow, data, weight_mask=wm, chan_mask_a=ca, want_valid=True, want_dst_flags=True)
    finally:
        _native.set_splat_path(0)
        _native.set_splat_pass_images(0)
    expect = _native.flow_flags(out[0], out[1])
    assert out[4].cpu().tolist() == expect.cpu().tolist()
    assert out1[4].cpu().tolist() == _native.flow_flags(out1[0], out1[1]).cpu().tolist()
    if kind == "zero":
        assert all((f & _native.FLAG_NZ) == 0 for f in out[4].cpu().tolist())
    if kind == "tiny":
        assert all((f & _native.FLAG_NZ) != 0 and (f & _native.FLAG_NZ_THR) == 0 for f in out[4].cpu().tolist())


@pytest.mark.parametrize("kind", ["routed", "general_path", "two_pass_inside", "narrow"])
def test_splat_of_a_difference_equals_the_materialised_difference(kind, dev):
    """`data_b`: the splat of data - data_b formed inside the kernels (gather kernel, un-occlude fill, two-pass fallback)
    is bit-identical to splatting the materialised difference -- combine_with mode 2 ('s') relies on it."""
    from oflibpytorch_amd import _native
    n, h, w = (2, 70, 132) if kind != "narrow" else (2, 20, 3)
    flow = _smooth(n, h, w, 1.5 if kind != "two_pass_inside" else 400.0, 9, dev)
    flow[0, :, : h // 3] = 0                                  # un-occlude fill candidates
    a, b = _smooth(n, h, w, 3.0, 10, dev), _smooth(n, h, w, 2.0, 11, dev)
    g = torch.Generator().manual_seed(5)
    wm = (torch.rand(n, h, w, generator=g) > 0.2).to(dev)
    kw = dict(weight_mask=wm, chan_mask_a=wm, want_valid=True, want_density=True)
    try:
        if kind == "general_path":
            _native.set_splat_path(1)
        fused = _native.splat_fwd(flow, a, data_b=b, **kw)
        plain = _native.splat_fwd(flow, a - b, **kw)
    finally:
        _native.set_splat_path(0)
    if kind in ("two_pass_inside", "general_path", "narrow"):  # float atomics (W < 4 takes the two-pass path too): order differs from run to run
        np.testing.assert_allclose(fused[0].cpu().numpy(), plain[0].cpu().numpy(), rtol=3e-5, atol=3e-4)
    else:
        assert torch.equal(fused[0], plain[0])
    assert torch.equal(fused[1], plain[1])


@pytest.mark.parametrize("shape", [(2, 3, 70, 132), (1, 1, 37, 50), (2, 4, 33, 47), (1, 3, 16, 4), (2, 3, 9, 3), (1, 3, 300, 400)])
@pytest.mark.parametrize("kind", ["smooth", "huge", "generic"])
def test_uint8_images_are_warped_from_their_bytes(shape, kind, dev):
    """ofl_warp_bwd_u8 (uint8 source read as bytes, float or uint8 destination) against the float kernel on the converted
    image: identical rounded values, identical valid mask -- including boxes that leave the LDS, narrow frames (binding
    falls back to the conversion) and more than 3 channels."""
    from oflibpytorch_amd import _native
    n, c, h, w = shape
    flow = _smooth(n, h, w, 1.5 if kind != "huge" else 300.0, 9, dev)
    g = torch.Generator().manual_seed(7)
    img = torch.randint(0, 256, (n, c, h, w), generator=g, dtype=torch.uint8).to(dev)
    sm = (torch.rand(n, h, w, generator=g) > 0.2).to(dev)
    try:
        if kind == "generic":
            _native.set_warp_path(1)
        for rm in (_native.ROUND_U8, _native.ROUND_NONE):
            kw = dict(src_mask=sm, flow_mask=sm, want_valid=True, round_mode=rm)
            ref = _native.warp_bwd(flow, img.float(), **kw)
            got = _native.warp_bwd(flow, img, **kw)
            assert got[0].dtype == torch.float32 and torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
            got8 = _native.warp_bwd(flow, img, out_uint8=True, **kw)
            if rm == _native.ROUND_U8 and kind != "generic" and w >= 4 and h >= 2:
                assert got8[0].dtype == torch.uint8
            assert torch.equal(got8[0].float(), ref[0]) and torch.equal(got8[1], ref[1])
    finally:
        _native.set_warp_path(0)


def test_flow_apply_on_a_uint8_image(dev):
    import oflibpytorch_amd as ofl
    n, h, w = 2, 96, 160
    g = torch.Generator().manual_seed(13)
    img = torch.randint(0, 256, (n, 3, h, w), generator=g, dtype=torch.uint8).to(dev)
    f = ofl.Flow(_smooth(n, h, w, 2.0, 20, dev), 't')
    out, valid = f.apply(img, return_valid_area=True)
    ref, rvalid = f.apply(img.float(), return_valid_area=True)
    assert torch.equal(out.float(), torch.clamp(torch.round(ref), 0, 255)) and torch.equal(valid, rvalid)
    assert torch.equal(ofl.apply_flow(f.vecs, img, 't').float(), torch.clamp(torch.round(ref), 0, 255))
    assert ofl.apply_flow(f.vecs, img, 't').dtype == torch.uint8


@pytest.mark.parametrize("shape", [(2, 70, 132), (1, 37, 50), (2, 9, 3), (1, 300, 400)])
@pytest.mark.parametrize("kind", ["smooth", "huge", "generic"])
def test_warp_of_a_difference_equals_the_materialised_difference(shape, kind, dev):
    """`src_b`: gathering src - src_b (subtracted while the box is staged, or per tap when the box does not fit the LDS)
    is bit-identical to gathering the materialised difference; shapes / paths the kernel variant does not cover are
    materialised by the binding."""
    from oflibpytorch_amd import _native
    n, h, w = shape
    flow = _smooth(n, h, w, 1.5 if kind != "huge" else 300.0, 9, dev)
    a, b = _smooth(n, h, w, 3.0, 10, dev), _smooth(n, h, w, 2.0, 11, dev)
    g = torch.Generator().manual_seed(5)
    sm = (torch.rand(n, h, w, generator=g) > 0.2).to(dev)
    kw = dict(src_mask=sm, flow_mask=sm, want_valid=True)
    try:
        if kind == "generic":
            _native.set_warp_path(1)
        fused = _native.warp_bwd(flow, a, src_b=b, **kw)
        plain = _native.warp_bwd(flow, a - b, **kw)
    finally:
        _native.set_warp_path(0)
    assert torch.equal(fused[0], plain[0]) and torch.equal(fused[1], plain[1])


def test_mode1_t_is_the_composed_expression(dev):
    import oflibpytorch_amd as ofl
    n, h, w = 2, 96, 160
    g = torch.Generator().manual_seed(12)
    m1 = (torch.rand(n, h, w, generator=g) > 0.1).to(dev)
    m2 = (torch.rand(n, h, w, generator=g) > 0.1).to(dev)
    A, B = ofl.Flow(_smooth(n, h, w, 1.5, 20, dev), 't', m1), ofl.Flow(_smooth(n, h, w, 2.0, 21, dev), 't', m2)
    x, y = A.combine_with(B, 1), A.invert().apply(B - A)
    assert torch.equal(x.vecs, y.vecs) and torch.equal(x.mask, y.mask) and x.ref == y.ref == 't'


def test_mode2_s_is_the_composed_expression(dev):
    import oflibpytorch_amd as ofl
    n, h, w = 2, 96, 160
    g = torch.Generator().manual_seed(12)
    m1 = (torch.rand(n, h, w, generator=g) > 0.1).to(dev)
    m2 = (torch.rand(n, h, w, generator=g) > 0.1).to(dev)
    A, B = ofl.Flow(_smooth(n, h, w, 1.5, 20, dev), 's', m1), ofl.Flow(_smooth(n, h, w, 2.0, 21, dev), 's', m2)
    x, y = A.combine_with(B, 2), A.apply(B - A)
    assert torch.equal(x.vecs, y.vecs) and torch.equal(x.mask, y.mask) and x.ref == y.ref == 's'


@pytest.mark.parametrize("rough", [False, True])
def test_routed_splat_in_several_passes(rough, dev):
    """n = 5 images, at most 2 per pass: the passes re-use the lists; with a rough flow the per-image two-pass fallback
    runs per pass.  Same results as one pass / as the two-pass path."""
    from oflibpytorch_amd import _native
    _native.collect_splat_stats = True
    n, c, h, w = 5, 3, 160, 320
    flow = _smooth(n, h, w, 2.0, 77, dev)
    if rough:
        # a ten-fold compression of the frame: the tiles it lands on list several times their capacity (whatever the tile width of
        # the build): every image is flagged
        xs = torch.arange(w, dtype=torch.float32, device=dev).view(1, 1, 1, w)
        ys = torch.arange(h, dtype=torch.float32, device=dev).view(1, 1, h, 1)
        flow = flow + torch.cat([(-0.9 * (xs - 150.3)).expand(n, 1, h, w), (-0.9 * (ys - 70.7)).expand(n, 1, h, w)], 1)
    g = torch.Generator().manual_seed(12)
    data = (torch.rand(n, c, h, w, generator=g) * 100 - 20).to(dev)
    wm = (torch.rand(n, h, w, generator=g) > 0.15).to(dev)
    kw = dict(weight_mask=wm, chan_mask_a=wm, want_mask_chan=True, want_density=True, want_warped=True)
    one = _native.splat_fwd(flow, data, **kw)
    assert int(_native._last_splat_stats[0].item()) == int(rough)
    _native.set_splat_pass_images(2)
    try:
        many = _native.splat_fwd(flow, data, **kw)
    finally:
        _native.set_splat_pass_images(0)
    for a, b in zip(one, many):
        if rough and a.dtype != torch.bool:
            np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=3e-5, atol=3e-3)   # float atomics
        else:
            assert torch.equal(a, b)


@pytest.mark.parametrize("pass_images", [0, 1])
def test_only_the_flagged_image_leaves_the_exact_path(pass_images, dev):
    """ADVICE r1 (overflow state must not leak between passes / images): image 0 of the batch overflows its lists and takes
    the two-pass path; images 1 and 2 -- in the same pass or in later passes -- stay on the in-order path: bit-identical
    to a call without image 0."""
    from oflibpytorch_amd import _native
    _native.collect_splat_stats = True
    n, c, h, w = 3, 2, 160, 320
    flow = _smooth(n, h, w, 2.0, 78, dev)
    xs = torch.arange(w, dtype=torch.float32, device=dev).view(1, 1, w)
    ys = torch.arange(h, dtype=torch.float32, device=dev).view(1, h, 1)
    flow[0] += torch.cat([(-0.9 * (xs - 150.3)).expand(1, h, w), (-0.9 * (ys - 70.7)).expand(1, h, w)], 0)   # ten-fold compression: its lists overflow
    g = torch.Generator().manual_seed(13)
    data = (torch.rand(n, c, h, w, generator=g) * 100 - 20).to(dev)
    wm = (torch.rand(n, h, w, generator=g) > 0.15).to(dev)
    kw = dict(want_density=True, want_warped=True)
    alone = _native.splat_fwd(flow[1:].contiguous(), data[1:].contiguous(), weight_mask=wm[1:].contiguous(), **kw)
    st = _native._last_splat_stats.cpu().tolist()
    assert st[0] == 0 and st[1] == 0
    _native.set_splat_pass_images(pass_images)
    try:
        mixed = _native.splat_fwd(flow, data, weight_mask=wm, **kw)
    finally:
        _native.set_splat_pass_images(0)
    st = _native._last_splat_stats.cpu().tolist()
    assert st[0] == 1 and st[2] == 1                           # exactly one image on the two-pass path
    for a, b in zip(alone, mixed):
        if a is not None:
            assert torch.equal(a, b[1:])


def test_tiled_splat_explicit_positions(dev):
    from oflibpytorch_amd import _native
    from oracle import oracle
    g = torch.Generator().manual_seed(4)
    n, c, h, w = 2, 3, 40, 64
    x = torch.rand(n, h, w, generator=g) * (w + 6) - 3
    y = torch.rand(n, h, w, generator=g) * (h + 6) - 3
    data = torch.rand(n, c, h, w, generator=g) * 50
    m = torch.rand(n, h, w, generator=g) > 0.2
    out, _, den, _ = _native.splat_fwd(None, data.to(dev), xs=x.to(dev), ys=y.to(dev), weight_mask=m.to(dev),
                                       occlude=False, want_density=True)
    ref, rden = oracle.grid_from_unstructured_data(x.numpy(), y.numpy(), data.numpy(), m.numpy())
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=3e-5, atol=3e-3)
    np.testing.assert_allclose(den.cpu().numpy(), rden, rtol=3e-5, atol=1e-5)


@pytest.mark.parametrize("ref", ["t", "s"])
@pytest.mark.parametrize("shape,pad", [((2, 3, 70, 132), [3, 5, 4, 2]), ((1, 2, 40, 61), [0, 7, 9, 0]), ((3, 1, 33, 47), [6, 0, 0, 5]),
                                       ((2, 3, 150, 260), [11, 13, 17, 19])])
def test_padded_apply_reads_the_flow_through_a_window(ref, shape, pad, dev):
    """Flow.apply(target, padding=...) -- the kernels read the un-padded flow through a window (zeros / replicate, mask False
    outside: ofl_warp_bwd_win_f32, ofl_splat_tiled_win_f32) -- against the same call on a materialised padded flow
    (`Flow.pad`, the reference's own route, flow_class.py:901-913): bit-identical values and masks, cut or not, with and
    without `consider_mask`, tensor and Flow targets."""
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _native
    n, c, hp, wp = shape
    h, w = hp - pad[0] - pad[1], wp - pad[2] - pad[3]
    g = torch.Generator().manual_seed(21)
    f = _smooth(n, h, w, 3.0, 5, dev)
    f[0, :, : h // 4] = 0                                            # zero-flow block (occlusion / un-occlude rule)
    m = (torch.rand(n, h, w, generator=g) > 0.15).to(dev)
    img = (torch.rand(n, c, hp, wp, generator=g) * 200).to(dev)
    tm = (torch.rand(n, hp, wp, generator=g) > 0.1).to(dev)
    fl = ofl.Flow(f, ref, m)
    padded = fl.pad(pad, mode='constant' if ref == 't' else 'replicate')
    _native.collect_splat_stats = True
    for cut in (True, False):
        for cons in (True, False):
            got = fl.apply(img, target_mask=tm.clone(), return_valid_area=True, consider_mask=cons, padding=pad, cut=cut)
            exact = ref == 't' or _native._last_splat_stats.cpu().tolist()[:2] == [0, 0]
            exp = padded.apply(img, target_mask=tm.clone(), return_valid_area=True, consider_mask=cons)
            if cut:
                exp = tuple(e[..., pad[0]:pad[0] + h, pad[2]:pad[2] + w] for e in exp)
            assert torch.equal(got[1], exp[1]), (cut, cons)
            if exact:
                assert torch.equal(got[0], exp[0]), (cut, cons)
            else:
                np.testing.assert_allclose(got[0].cpu().numpy(), exp[0].cpu().numpy(), rtol=3e-5, atol=3e-3)
    tf = ofl.Flow(_smooth(n, hp, wp, 2.0, 6, dev), ref, tm)
    got = fl.apply(tf, padding=pad, cut=False)
    exp = padded.apply(tf)
    assert torch.equal(got.vecs, exp.vecs) and torch.equal(got.mask, exp.mask)
    got8 = fl.apply((img).to(torch.uint8), padding=pad)              # integer targets: rounded in the kernel
    exp8 = padded.apply((img).to(torch.uint8))[..., pad[0]:pad[0] + h, pad[2]:pad[2] + w]
    assert torch.equal(got8, exp8)


@pytest.mark.parametrize("shape", [(3, 70, 132), (2, 37, 50), (2, 64, 96), (1, 33, 47)])
def test_fp16_stored_flows_are_read_directly(shape, dev):
    """BASELINE config 5 storage: a Flow handed over in fp16 keeps its halves; `switch_ref`, `invert`, `Flow.apply(Flow)` ('s':
    ofl_splat_tiled_f16) and `combine_with` mode 1 't' (ofl_warp_bwd_h_f32: the fp16 flow is the gathered source) read them
    directly.  Everything must be bit-identical to the same calls on the up-cast fp32 tensors -- the reference's `.float()`
    on entry (utils.py:95, 118) -- values, masks, references and flag words."""
    import oflibpytorch_amd as ofl
    n, h, w = shape
    g = torch.Generator().manual_seed(9)
    f16 = _smooth(n, h, w, 2.5, 31, dev).half()
    f16[0, :, : h // 3] = 0
    g16 = _smooth(n, h, w, 1.5, 32, dev).half()
    m = (torch.rand(n, h, w, generator=g) > 0.2).to(dev)
    m2 = (torch.rand(n, h, w, generator=g) > 0.2).to(dev)
    for ref in 'st':
        a16, a32 = ofl.Flow(f16, ref, m), ofl.Flow(f16.float(), ref, m)
        b16, b32 = ofl.Flow(g16, ref, m2), ofl.Flow(g16.float(), ref, m2)
        assert a16._half is not None and a16._v32 is None            # no fp32 copy was made at construction
        assert a16._flags() == a32._flags()
        pairs = [(a16.switch_ref(), a32.switch_ref()), (a16.invert(), a32.invert()),
                 (a16.invert('s' if ref == 't' else 't'), a32.invert('s' if ref == 't' else 't')),
                 (a16.apply(b16), a32.apply(b32))]
        pairs += [(a16.combine_with(b16, mode), a32.combine_with(b32, mode)) for mode in (1, 2, 3)]
        for x, y in pairs:
            assert x.ref == y.ref and x.vecs.dtype == torch.float32
            assert torch.equal(x.vecs, y.vecs) and torch.equal(x.mask, y.mask)
            assert x._flags() == y._flags()
    assert a16.vecs.dtype == torch.float32 and torch.equal(a16.vecs, f16.float())     # `.vecs` hands out fp32, like the reference


def test_fp16_flow_outputs_are_an_option(dev):
    """`set_half_flow_outputs(True)`: a flow produced from fp16-stored flows by the splat family is STORED in fp16 (fp32
    arithmetic, one round-to-nearest-even at the store) and stays in fp16 down a chain; values = the fp32 result rounded to
    fp16, masks identical, flag words those of the stored values.  Off by default."""
    import oflibpytorch_amd as ofl
    n, h, w = 2, 96, 160
    f16 = _smooth(n, h, w, 2.5, 41, dev).half()
    m = (torch.rand(n, h, w, generator=torch.Generator().manual_seed(4)) > 0.15).to(dev)
    ref32 = ofl.Flow(f16, 's', m).switch_ref()
    assert ref32._half is None
    try:
        ofl.set_half_flow_outputs(True)
        out = ofl.Flow(f16, 's', m).switch_ref()
        assert out._half is not None and out._v32 is None and out.ref == 't'
        assert torch.equal(out._half, ref32.vecs.half()) and torch.equal(out.mask, ref32.mask)
        assert out._flags() == ofl.Flow(ref32.vecs.half(), 't', ref32.mask)._flags()
        again = out.invert()                                          # the chain stays in fp16 storage
        assert again._half is not None
        assert torch.equal(again._half, ofl.Flow(out._half.float(), 't', out.mask).invert().vecs.half())
    finally:
        ofl.set_half_flow_outputs(False)
    assert ofl.Flow(f16, 's', m).switch_ref()._half is None


@pytest.mark.gpu
def test_flag_words_or_for_the_sharded_reduce(dev):
    """ofl_flag_words_or_i32: the words come back unchanged, followed by the bits of their OR (what
    distributed.with_global_or all-reduces); N from 1 to beyond one wave."""
    from oflibpytorch_amd import _native, distributed
    g = torch.Generator().manual_seed(3)
    for n in (1, 2, 5, 64, 65, 300):
        words = torch.randint(0, 32, (n,), generator=g, dtype=torch.int32)
        if n > 2:
            words &= 0b10110                                  # two bits never set
        out = _native.flag_words_or(words.to(dev)).cpu().tolist()
        expect = 0
        for v in words.tolist():
            expect |= v
        assert out[:n] == words.tolist() and out[n:] == [(expect >> k) & 1 for k in range(5)]
        assert distributed.split_global_or(distributed.with_global_or(words.to(dev)).cpu().tolist()) == (words.tolist(), expect)


def _splat_sum_reference(flow, data, flow_sign, data_sign):
    """ofl_splat_sum_f32 restated with loops (small frames): per corner class, in raster order of the source pixels, then
    ((c0 + c1) + c2) + c3 -- the order of utils.py:1133-1143 without the division of :1144.  The end point is the backward warp's
    sample position: grid + flow_sign * flow through normalise_coords and the grid sampler's un-normalise (the weights of the
    gradient are the forward's)."""
    n, c, h, w = data.shape
    out = np.zeros((n, c, h, w), np.float32)
    f32 = np.float32

    def position(p, size):
        g = f32(f32(f32(p * f32(2)) / f32(size - 1)) - f32(1))
        return f32(f32(g + f32(1)) * f32(f32(size - 1) / f32(2)))
    for b in range(n):
        acc = np.zeros((4, c, h, w), np.float32)
        for y in range(h):
            for x in range(w):
                xv = position(f32(f32(flow_sign) * flow[b, 0, y, x] + f32(x)), w)
                yv = position(f32(f32(flow_sign) * flow[b, 1, y, x] + f32(y)), h)
                x0, y0 = np.floor(xv), np.floor(yv)
                for ky in range(2):
                    for kx in range(2):
                        xi, yi = int(x0) + kx, int(y0) + ky
                        if not (0 <= xi < w and 0 <= yi < h):
                            continue
                        wx = f32(f32(x0 + 1) - xv) if kx == 0 else f32(xv - f32(x0))
                        wy = f32(f32(y0 + 1) - yv) if ky == 0 else f32(yv - f32(y0))
                        wgt = f32(wy * wx)
                        for ch in range(c):
                            acc[2 * ky + kx, ch, yi, xi] = f32(acc[2 * ky + kx, ch, yi, xi] + f32(wgt * f32(f32(data_sign) * data[b, ch, y, x])))
        out[b] = ((acc[0] + acc[1]) + acc[2]) + acc[3]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 40, 56), (1, 5, 33, 45), (2, 2, 64, 72)])
def test_splat_sum_is_the_unnormalised_splat_bit_for_bit(shape, dev):
    """ofl_splat_sum_f32 (the gradient of the backward warp wrt its source) against its loop restatement: bit-exact on a
    fold-free flow, both signs, more than three channels, odd widths.  (The restatement's end points are the warp's sample
    positions since tests/test_gpu_grad_oracle64.py found the weights off by the position's rounding.)"""
    from oflibpytorch_amd import _native
    _native.collect_splat_stats = True
    n, c, h, w = shape
    g = torch.Generator().manual_seed(c + h)
    flow = _smooth(n, h, w, 1.5, 91, dev)
    data = (torch.rand(n, c, h, w, generator=g) * 10 - 3)
    for fs, ds in ((1.0, 1.0), (-1.0, -1.0)):
        got = _native.splat_sum(flow, data.to(dev), flow_sign=fs, data_sign=ds)
        st = _native._last_splat_stats.cpu().tolist()
        assert st[0] == 0 and st[1] == 0
        assert np.array_equal(got.cpu().numpy(), _splat_sum_reference(flow.cpu().numpy(), data.numpy(), fs, ds))


@pytest.mark.parametrize("case", ["apply", "apply_novalid", "mode3", "bcast_src", "bcast_flow", "sign"])
def test_lean_binding_equals_the_general_one(case):
    """`_native._warp_bwd_lean` (the short host path of the plain fp32 warp: Flow.apply 't', combine_with) hands the C ABI the same
    arguments as `_warp_bwd_raw`: same results, bit for bit, incl. batch broadcasts of either operand and the addend / sign epilogue."""
    import torch
    from oflibpytorch_amd import _native
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(91)
    n, c, h, w = 3, 3, 70, 100
    flow = (torch.randn(n, 2, h, w, generator=g) * 4).to(dev)
    src = torch.rand(n, c, h, w, generator=g).to(dev)
    sm = (torch.rand(n, h, w, generator=g) > 0.2).to(dev)
    fm = (torch.rand(n, h, w, generator=g) > 0.2).to(dev)
    kw = dict(src_mask=sm, flow_mask=fm, want_valid=True)
    if case == "apply_novalid":
        kw = dict(src_mask=None, flow_mask=None, want_valid=False)
    elif case == "mode3":
        src = (torch.randn(n, 2, h, w, generator=g) * 3).to(dev)
        kw.update(addend=flow, a_sign=1.0, g_sign=1.0)
    elif case == "bcast_src":
        src, kw["src_mask"] = src[:1].contiguous(), sm[:1].contiguous()
    elif case == "bcast_flow":
        flow, kw["flow_mask"] = flow[:1].contiguous(), fm[:1].contiguous()
    elif case == "sign":
        src = (torch.randn(n, 2, h, w, generator=g) * 3).to(dev)
        kw.update(flow_sign=-1.0, addend=src, a_sign=-1.0, g_sign=1.0)
    lean = _native._warp_bwd_lean(flow, src, **kw)
    assert lean is not None, "the plain contiguous fp32 call must take the short path"
    with torch.cuda.device(dev):
        full = _native._warp_bwd_raw(flow, src, **kw)
    for a, b in zip(lean, full):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.shape == b.shape and a.dtype == b.dtype
            assert torch.equal(a, b) or bool(((a == b) | (a.isnan() & b.isnan())).all())
    # and the calls it must leave to the general path
    assert _native._warp_bwd_lean(flow, src, round_mode=_native.ROUND_U8, **kw) is None
    assert _native._warp_bwd_lean(flow.transpose(2, 3).contiguous().transpose(2, 3), src, **kw) is None


# ------------------------------------------------------------------------------------------------------------------------
# round 4: the valid area of a backward warp in one launch (ofl_warp_valid_f32), Flow.combine as one fused launch per cell
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 37, 53), (1, 64, 128), (3, 90, 142), (1, 300, 400), (2, 1080, 1920)])
def test_warp_valid_matches_a_warped_ones_image_and_the_oracle(shape, dev):
    """`(G(sign * f, ones) > 0.9999) & mask` from ofl_warp_valid_f32 (no image) == the same through the warp kernel on a real
    all-ones image == the oracle; vector (W % 4 == 0) and scalar instantiations, both signs, with and without a mask."""
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _native
    from oracle import oracle
    n, h, w = shape
    g = torch.Generator().manual_seed(n * h + w)
    lo = torch.randn(n, 2, max(h // 20, 2), max(w // 20, 2), generator=g) * 9
    f = torch.nn.functional.interpolate(lo, size=(h, w), mode='bicubic', align_corners=True).contiguous()
    f[:, :, : h // 6] = 0.0                                   # an identity band: every tap weight 0 or 1
    f[:, 0, h // 3: h // 3 + 4] = torch.round(f[:, 0, h // 3: h // 3 + 4])   # integer shifts: samples on pixel centres
    m = torch.rand(n, h, w, generator=g) > 0.1
    ones = torch.ones(n, 1, h, w)
    for sign in (1.0, -1.0):
        for mask in (m, None):
            got = _native.warp_valid(f.to(dev), None if mask is None else mask.to(dev), sign, 0.9999).cpu().numpy()
            via_image = _native.warp_bwd(f.to(dev), ones.to(dev), flow_sign=sign)[0][:, 0].cpu() > 0.9999
            exp = oracle.G(f.numpy() * np.float32(sign), ones.numpy())[:, 0] > np.float32(0.9999)
            if mask is not None:
                via_image, exp = via_image & mask, exp & mask.numpy()
            assert np.array_equal(got, exp), "ofl_warp_valid_f32 differs from the oracle (sign %g)" % sign
            assert np.array_equal(got, via_image.numpy()), "ofl_warp_valid_f32 differs from the warped ones image"
    fl = ofl.Flow(f.to(dev), 't', m.to(dev))
    assert np.array_equal(fl.valid_target().cpu().numpy(), (oracle.G(f.numpy(), ones.numpy())[:, 0] > np.float32(0.9999)) & m.numpy())
    fs = ofl.Flow(f.to(dev), 's', m.to(dev))
    assert np.array_equal(fs.valid_source().cpu().numpy(), (oracle.G(-f.numpy(), ones.numpy())[:, 0] > np.float32(0.9999)) & m.numpy())


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_fused_combine_equals_the_operator_chain(mode, dev):
    """Every (self.ref, other.ref, ref) cell of Flow.combine: the fused plan (addend epilogue of the gather / difference formed
    inside the splat, negations as kernel signs) == the same plan through apply / * / + (one launch per operator), bit for bit,
    and == the oracle-backed host logic's result is what tests/test_host_logic_golden.py pins on the fixtures."""
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import flow_class
    n, h, w = 2, 150, 212
    g = torch.Generator().manual_seed(40 + mode)
    mk = lambda s: torch.nn.functional.interpolate(torch.randn(n, 2, 5, 6, generator=g) * s, size=(h, w), mode='bicubic', align_corners=True).contiguous()
    f1, f2 = mk(3.0).to(dev), mk(2.0).to(dev)
    m1 = (torch.rand(n, h, w, generator=g) > 0.05).to(dev)
    m2 = (torch.rand(n, h, w, generator=g) > 0.05).to(dev)
    try:
        for sr in 'st':
            for orf in 'st':
                for ref in 'st':
                    a, b = ofl.Flow(f1, sr, m1), ofl.Flow(f2, orf, m2)
                    flow_class._COMBINE_FUSED = False
                    chain = a.combine(b, mode, ref)
                    flow_class._COMBINE_FUSED = True
                    fused = a.combine(b, mode, ref)
                    assert fused.ref == chain.ref == ref
                    assert torch.equal(fused.mask, chain.mask), (mode, sr, orf, ref)
                    assert torch.equal(fused.vecs, chain.vecs), (mode, sr, orf, ref)
    finally:
        flow_class._COMBINE_FUSED = True
