"""GPU tier: every gradient kernel against the float64 oracle of tests/grad_oracle64.py, element by element.

    |got - ref64| <= (k + r) * 2^-24 * M + (k + r) * 2^-126        on EVERY element (r: grad_oracle64.R, licensed by ATen's own
                                                                   float32 autograd in tests/test_grad_oracle64_host.py)

`_native` is called directly and every case asserts `last_kernel_name()` first, so no case can silently test another kernel.
Inputs: the five flow families and the upstream gradient of tests/grad_cases64.py (taps leaving every border, whole rows
outside, integer positions, exactly-zero discs, gradients of 1e-4 ... 1 side by side), flow_sign +1 and -1, g_scale 0.5, on the
smallest frames that cross every boundary of the kernels (ragged and exact tiles, W % 4 != 0, W < 4).

  * ofl_warp_bwd_grad_f32: warp_grad_kernel (path 1, W = 3, C = 5), the row-table GRAD kernel with one tile per block (automatic at
    these sizes) and four (path 7), the column GRAD kernel (path 6 and the W = 70 frame) -- want_src alone, want_flow alone, both.
    grad_src on the route the binding takes: float atomics (W < 4) or ofl_splat_sum_f32.
  * ofl_warp_bwd_grad_x16 (fp16, bf16) and ofl_warp_bwd_grad_nhwc (fp32, fp16, bf16; C a multiple of 4, as the binding asks):
    grad_flow, on the exactly widened inputs, with the same float32 bar.
  * ofl_splat_grad_f32: C = 1, 2, 3, 5 (two groups), with and without holes, occlusion on and off, with a density gradient,
    explicit end points; `out` and `density` from the package's own forward on the device.
  * ofl_sample_pts_grad_f32: 257 points (frame corners, integers, outside, a NaN row, 64 in one cell), batch-1 points under N flows.

With OFL_GRAD_ORACLE64_JSON set to a path, the largest err / bound met per kernel and output is written there (a record of
margin -- profiles/grad_oracle64.json -- nothing asserts on it).
"""
import json
import os
import re

import numpy as np
import pytest
import torch

import grad_cases64 as gc
import grad_oracle64 as go

pytestmark = pytest.mark.gpu

CL = torch.channels_last
TAG = {torch.float32: "float", torch.float16: "half_t", torch.bfloat16: "bf16_t"}
MARGINS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tier needs a HIP device"
    from oflibpytorch_amd import _native
    _native.load_library()
    return torch.device('cuda', 0)


def _kernel():
    from oflibpytorch_amd import _native
    return _native.last_kernel_name()


def _label(name):
    m = re.search(r"(\w+_kernel)(?:<(\d+|true|false|\w+_t|float)\b)?", name)
    return name if m is None else (m.group(1) if m.group(2) is None else "%s<%s>" % m.groups())


class Report(object):
    """Collects err / bound of every comparison of a test, prints each figure, and fails at the end on the worst one."""

    def __init__(self):
        self.bad = []

    def check(self, got, ref, key, label, what):
        ex = go.excess(got.detach().float().cpu().numpy(), ref, go.R[key])
        slot = MARGINS.setdefault(label, {})
        slot[key] = max(slot.get(key, 0.0), ex)
        print("%-72s %-16s %-34s err/bound %.4g" % (what, key, label, ex))
        if not ex <= 1.0:
            self.bad.append("%s %s on %s: |got - ref64| reaches %.4g of the per-element bound (r = %d)" % (what, key, label, ex, go.R[key]))

    def done(self):
        path = os.environ.get("OFL_GRAD_ORACLE64_JSON")
        if path:
            with open(path, "w") as fh:
                json.dump({k: {o: float("%.4g" % v) for o, v in sorted(d.items())} for k, d in sorted(MARGINS.items())}, fh, indent=1)
        assert not self.bad, "\n".join(self.bad)


# ------------------------------------------------------------------------------------------------
# ofl_warp_bwd_grad_f32
# ------------------------------------------------------------------------------------------------
ROWS1, ROWS4, COLUMN, LANE = r"warp_bwd_rows_kernel<1, %d,", r"warp_bwd_rows_kernel<4, %d,", r"warp_bwd_lds_column_kernel<\d+, %d,", "warp_grad_kernel"
WARP_CASES = [((2, 37, 70), 0, COLUMN), ((2, 37, 70), 6, COLUMN), ((2, 37, 70), 1, LANE),
              ((2, 64, 128), 0, ROWS1), ((2, 64, 128), 7, ROWS4), ((2, 64, 128), 6, COLUMN), ((2, 64, 128), 1, LANE),
              ((1, 17, 68), 0, ROWS1), ((1, 17, 68), 7, ROWS4), ((1, 17, 68), 1, LANE),
              ((2, 9, 3), 0, LANE)]


def _flow_kernel_ok(pattern, c, name):
    return re.search(pattern % c if "%d" in pattern else pattern, name) is not None


@pytest.mark.parametrize("family", gc.FAMILIES)
@pytest.mark.parametrize("shape,path,pattern", WARP_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_warp_gradients(shape, path, pattern, family, dev):
    from oflibpytorch_amd import _native
    n, h, w = shape
    rep = Report()
    f0 = gc.flow(family, n, h, w)
    _native.set_warp_path(path)
    try:
        for c in (1, 2, 3, 5):
            # more than 3 channels: the one-pixel-per-lane kernel whatever the path
            pat = LANE if c > 3 else pattern
            variants = [(f0, gc.image(n, c, h, w))]
            if n > 1 and c == 2:
                variants += [(f0[:1].contiguous(), gc.image(n, c, h, w)), (f0, gc.image(1, c, h, w))]     # batch-1 flow; batch-1 source
            gout = gc.upstream(n, c, h, w)
            for fl, src in variants:
                for sign in (1.0, -1.0):
                    ref = go.warp_grad(fl.numpy(), src.numpy(), gout.numpy(), sign, gc.G_SCALE)
                    what = "%s %s path %d C=%d flow %d src %d sign %+d" % (family, shape, path, c, fl.shape[0], src.shape[0], sign)
                    for want_src, want_flow in ((True, False), (False, True), (True, True)):
                        gs, gf = _native.warp_bwd_grad(fl.to(dev), src.to(dev), gout.to(dev), flow_sign=sign, g_scale=gc.G_SCALE,
                                                       want_src=want_src, want_flow=want_flow)
                        name = _kernel()
                        mode = what + (" src" if want_src else "") + (" flow" if want_flow else "")
                        if want_flow:
                            assert _flow_kernel_ok(pat, c, name), (mode, name)
                            rep.check(gf, ref['grad_flow'], 'warp.grad_flow', _label(name), mode)
                        else:
                            assert gf is None
                        if want_src:
                            if w < 4:
                                assert LANE in name, (mode, name)
                                route = "float atomics (warp_grad_kernel)"
                            else:
                                assert want_flow or "splat" in name, (mode, name)
                                route = "ofl_splat_sum_f32"
                            assert gs.shape == src.shape
                            rep.check(gs, ref['grad_src'], 'warp.grad_src', route, mode + " via " + route)
                        else:
                            assert gs is None
    finally:
        _native.set_warp_path(0)
    rep.done()


X16_FRAMES = [(2, 37, 70), (2, 64, 128), (1, 17, 68)]      # (frames of W < 4 are declined: the fp32 kernels take them)


@pytest.mark.parametrize("family", gc.FAMILIES)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("shape", X16_FRAMES, ids=str)
def test_warp_flow_gradient_of_16_bit_planes(shape, dtype, family, dev):
    from oflibpytorch_amd import _native
    n, h, w = shape
    rep = Report()
    f0 = gc.flow(family, n, h, w)
    for c in (1, 2, 3, 5):
        src, gout = gc.image(n, c, h, w).to(dtype), gc.upstream(n, c, h, w).to(dtype)
        for fl in ([f0, f0[:1].contiguous()] if (n > 1 and c == 2) else [f0]):
            for sign in (1.0, -1.0):
                res = _native.warp_bwd_grad_x16(fl.to(dev), src.to(dev), gout.to(dev), flow_sign=sign, g_scale=gc.G_SCALE,
                                                want_src=False, want_flow=True)
                name = _kernel()
                assert res is not None and res[0] is None
                assert TAG[dtype] in name and ("warp_grad_flow_x16_kernel" in name if c > 3 else
                                               ("warp_bwd_rows_kernel" in name or "warp_bwd_lds_column_kernel" in name)), name
                ref = go.warp_grad(fl.numpy(), src.float().numpy(), gout.float().numpy(), sign, gc.G_SCALE)
                m = re.search(r"(\w+_kernel)<(\d+)?", name)
                label = "%s<%s> %s" % (m.group(1), m.group(2) or "", TAG[dtype]) if c <= 3 else "warp_grad_flow_x16_kernel<%s>" % TAG[dtype]
                rep.check(res[1], ref['grad_flow'], 'warp.grad_flow', label,
                          "%s %s %s C=%d flow %d sign %+d" % (family, shape, TAG[dtype], c, fl.shape[0], sign))
    rep.done()


@pytest.mark.parametrize("family", gc.FAMILIES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("shape", gc.SHAPES, ids=str)
def test_warp_flow_gradient_of_channels_last_tensors(shape, dtype, family, dev):
    from oflibpytorch_amd import _native
    n, h, w = shape
    rep = Report()
    f0 = gc.flow(family, n, h, w)
    for c in (4, 8):                                        # (the channels_last route takes multiples of 4)
        src = gc.image(n, c, h, w).to(dtype).to(dev).contiguous(memory_format=CL)
        gout = gc.upstream(n, c, h, w).to(dtype).to(dev).contiguous(memory_format=CL)
        for fl in ([f0, f0[:1].contiguous()] if (n > 1 and c == 4) else [f0]):
            for sign in (1.0, -1.0):
                res = _native.warp_bwd_grad_nhwc(fl.to(dev), src, gout, flow_sign=sign, g_scale=gc.G_SCALE, want_src=False, want_flow=True)
                name = _kernel()
                assert res is not None and res[0] is None
                assert "warp_grad_flow_nhwc_kernel" in name and ("<float," if dtype == torch.float32 else TAG[dtype]) in name, name
                ref = go.warp_grad(fl.numpy(), src.float().cpu().numpy(), gout.float().cpu().numpy(), sign, gc.G_SCALE)
                rep.check(res[1], ref['grad_flow'], 'warp.grad_flow', "warp_grad_flow_nhwc_kernel<%s>" % TAG[dtype],
                          "%s %s %s C=%d flow %d sign %+d" % (family, shape, TAG[dtype], c, fl.shape[0], sign))
    rep.done()


# ------------------------------------------------------------------------------------------------
# ofl_splat_grad_f32
# ------------------------------------------------------------------------------------------------
def _splat_case(rep, dev, what, c, n, h, w, *, flow=None, xs=None, ys=None, sign=1.0, holes=False, occlude=True, with_gden=False,
                data_rows=None):
    from oflibpytorch_amd import _native
    data = gc.image(n if data_rows is None else data_rows, c, h, w)
    gout = (gc.upstream(n, c, h, w) * gc.G_SCALE).contiguous()
    gden = gc.upstream(n, 1, h, w, 1)[:, 0].contiguous() if with_gden else None
    m = gc.holes(n, h, w) if holes else None
    kw = dict(flow_sign=sign, weight_mask=None if m is None else m.to(dev), occlude=occlude)
    if flow is None:
        kw.update(xs=xs.to(dev), ys=ys.to(dev))
    fd = None if flow is None else flow.to(dev)
    out, _, den, _ = _native.splat_fwd(fd, data.to(dev), want_density=True, **kw)
    gd, gxy = _native.splat_grad(fd, data.to(dev), out, den, gout.to(dev), grad_density=None if gden is None else gden.to(dev), **kw)
    name = _kernel()
    assert "splat_grad_kernel" in name, name
    ref = go.splat_grad(None if flow is None else flow.numpy(), data.numpy(), out.cpu().numpy(), den.cpu().numpy(), gout.numpy(),
                        None if gden is None else gden.numpy(), None if m is None else m.numpy(), occlude, sign,
                        None if xs is None else xs.numpy(), None if ys is None else ys.numpy())
    rep.check(gd, ref['grad_data'], 'splat.grad_data', "splat_grad_prep_kernel + splat_grad_kernel", what)
    rep.check(gxy, ref['grad_xy'], 'splat.grad_xy', "splat_grad_prep_kernel + splat_grad_kernel", what)
    return ref


@pytest.mark.parametrize("family", gc.FAMILIES)
@pytest.mark.parametrize("shape", gc.SHAPES, ids=str)
def test_splat_gradients(shape, family, dev):
    n, h, w = shape
    rep = Report()
    f0 = gc.flow(family, n, h, w)
    for c in (1, 2, 3, 5):
        for i, (holes, occlude, with_gden) in enumerate([(False, True, False), (True, True, True), (True, False, False), (False, False, True)]):
            for sign in ((1.0, -1.0) if c == 3 else ((1.0, -1.0)[(i + c) % 2],)):
                what = "%s %s C=%d holes %d occlude %d gden %d sign %+d" % (family, shape, c, holes, occlude, with_gden, sign)
                _splat_case(rep, dev, what, c, n, h, w, flow=f0, sign=sign, holes=holes, occlude=occlude, with_gden=with_gden)
    if n > 1:                                               # a batch-1 flow and batch-1 data under N upstream gradients
        _splat_case(rep, dev, "%s %s batch-1 flow" % (family, shape), 3, n, h, w, flow=f0[:1].contiguous(), sign=-1.0, holes=True, with_gden=True)
        _splat_case(rep, dev, "%s %s batch-1 data" % (family, shape), 2, n, h, w, flow=f0, holes=True, data_rows=1)
    rep.done()


def test_splat_gradients_at_explicit_end_points(dev):
    n, c, h, w = 2, 5, 37, 70
    rep = Report()
    f0 = gc.flow('shift_pos', n, h, w)
    xs = (f0[:, 0] * 0.5 + torch.arange(w, dtype=torch.float32)[None, None, :]).contiguous()
    ys = (f0[:, 1] * 0.5 + torch.arange(h, dtype=torch.float32)[None, :, None]).contiguous()
    _splat_case(rep, dev, "explicit xs / ys C=5", c, n, h, w, xs=xs, ys=ys, holes=True, occlude=False, with_gden=True)
    rep.done()


# ------------------------------------------------------------------------------------------------
# ofl_sample_pts_grad_f32
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", gc.FAMILIES)
@pytest.mark.parametrize("shape", gc.SHAPES, ids=str)
def test_point_sampler_gradients(shape, family, dev):
    from oflibpytorch_amd import _native
    n, h, w = shape
    rep = Report()
    f0 = gc.flow(family, n, h, w)
    g = torch.Generator().manual_seed(6000)
    gout = (torch.randn(n, 257, 2, generator=g) * torch.logspace(-4, 0, 257).view(1, 257, 1)).contiguous()
    for rows in sorted({1, n}):                             # batch-1 points under N flows; N-M-2
        pts = gc.points(rows, h, w)
        ref = go.sample_pts_grad(f0.numpy(), pts.numpy(), gout.numpy())
        assert int(np.isnan(ref['grad_pts'][0]).sum()) == n
        for want_flow, want_pts in ((True, False), (False, True), (True, True)):
            gf, gp = _native.sample_pts_grad(f0.to(dev), pts.to(dev), gout.to(dev), want_flow=want_flow, want_pts=want_pts)
            name = _kernel()
            assert "sample_pts_kernel<true>" in name, name
            what = "%s %s point rows %d%s%s" % (family, shape, rows, " flow" if want_flow else "", " pts" if want_pts else "")
            if want_flow:
                rep.check(gf, ref['grad_flow'], 'pts.grad_flow', "sample_pts_kernel<true>", what)
            if want_pts:
                rep.check(gp, ref['grad_pts'], 'pts.grad_pts', "sample_pts_kernel<true>", what)
    rep.done()
