"""CPU tier of the channels_last backward (ofl_warp_bwd_grad_nhwc, ofl_nhwc_to_planes, ofl_planes_to_nhwc; DESIGN.md 3.14 "Autograd"):
the three entry points in the header and the built library, their argument checks (all of them come before anything touches a device),
and the routing predicate `_native._nhwc_grad_kind` on CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

from oflibpytorch_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CL = torch.channels_last
KIND = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}          # OFL_X16_HALF, OFL_X16_BFLOAT, OFL_NHWC_F32
E_NULL, E_SHAPE, E_ARG, E_UNSUPPORTED = -1, -2, -3, -4
P = ctypes.c_void_p


def _cl(n, c, h, w, dtype=torch.float32):
    t = torch.zeros(n, c, h, w, dtype=dtype).contiguous(memory_format=CL)
    assert t.data_ptr() % 64 == 0
    return t


def _args(text, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, "include/oflib_hip.h does not declare %s" % name
    return [a.strip().split()[-1].lstrip("*") for a in m.group(1).replace("\n", " ").split(",")]


def test_header_declares_the_entry_points_and_the_library_exports_them():
    text = open(os.path.join(ROOT, "include", "oflib_hip.h")).read()
    lib = _native.load_library()
    want = {"ofl_warp_bwd_grad_nhwc": ["flow", "flow_bs", "flow_sign", "src", "src_bs", "grad_out", "g_scale", "grad_flow",
                                       "n", "c", "h", "w", "dtype", "stream"],
            "ofl_nhwc_to_planes": ["src", "dst", "n", "c", "h", "w", "elem_bytes", "stream"],
            "ofl_planes_to_nhwc": ["src", "dst", "n", "c", "h", "w", "elem_bytes", "stream"]}
    for name, args in want.items():
        assert _args(text, name) == args, name
        assert name in _native.exported_symbols()
        assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == len(args)
    assert lib.ofl_version() == _native.ABI_VERSION == 36


@pytest.fixture(scope="module")
def base():
    buf = (ctypes.c_char * 8192)()
    yield (ctypes.addressof(buf) + 63) & ~63
    del buf


def test_the_flow_gradient_entry_point_rejects_and_declines_without_a_device(base):
    lib = _native.load_library()

    def call(n=2, c=8, h=5, w=7, dtype=2, flow=base, src=base + 1024, gout=base + 4096, gflow=base + 7168, flow_bs=70, src_bs=280,
             flow_sign=1.0):
        return lib.ofl_warp_bwd_grad_nhwc(P(flow), flow_bs, flow_sign, P(src), src_bs, P(gout), 1.0, P(gflow), n, c, h, w, dtype, None)
    assert call(flow=None) == E_NULL and call(src=None) == E_NULL and call(gout=None) == E_NULL and call(gflow=None) == E_NULL
    assert call(dtype=3) == E_ARG and call(dtype=-1) == E_ARG
    assert call(flow_bs=-1) == E_ARG and call(src_bs=-1) == E_ARG and call(n=-1) == E_ARG and call(c=-4) == E_ARG
    assert call(flow_sign=0.5) == E_ARG and call(flow_sign=0.0) == E_ARG
    assert call(n=0) == E_SHAPE
    for kw in (dict(c=6), dict(c=2), dict(c=3), dict(h=1), dict(w=1), dict(n=65536)):
        assert call(**kw) == E_UNSUPPORTED, kw
    for dtype, offs in ((2, (4, 8, 12)), (0, (2, 4, 6)), (1, (2, 4, 6))):
        for o in offs:
            assert call(dtype=dtype, src=base + 1024 + o) == E_UNSUPPORTED, (dtype, o)
            assert call(dtype=dtype, gout=base + 4096 + o) == E_UNSUPPORTED, (dtype, o)


@pytest.mark.parametrize("name", ["ofl_nhwc_to_planes", "ofl_planes_to_nhwc"])
def test_the_layout_copies_reject_and_decline_without_a_device(name, base):
    lib = _native.load_library()
    fn = getattr(lib, name)
    to_planes = name == "ofl_nhwc_to_planes"

    def call(n=2, c=8, h=5, w=7, elem=4, nhwc=base, planes=base + 4096):
        src, dst = (nhwc, planes) if to_planes else (planes, nhwc)
        return fn(P(src), P(dst), n, c, h, w, elem, None)
    assert call(nhwc=None) == E_NULL and call(planes=None) == E_NULL
    for elem in (0, 1, 3, 8, -2):
        assert call(elem=elem) == E_ARG, elem
    assert call(n=-1) == E_ARG and call(c=-4) == E_ARG
    assert call(n=0) == E_SHAPE and call(h=0) == E_SHAPE
    for kw in (dict(c=6), dict(c=2), dict(c=3), dict(c=6, elem=2), dict(n=65536)):
        assert call(**kw) == E_UNSUPPORTED, kw
    for elem, offs in ((4, (4, 8, 12)), (2, (2, 4, 6))):
        for o in offs:
            assert call(elem=elem, nhwc=base + o) == E_UNSUPPORTED, (elem, o)
    assert call(elem=4, planes=base + 4096 + 2) == E_ARG and call(elem=2, planes=base + 4096 + 1) == E_ARG   # not even element-aligned
    assert call(planes=base) == E_ARG and call(planes=base + 64) == E_ARG                                     # the operands overlap


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=str)
def test_a_matching_channels_last_pair_qualifies(dtype):
    for shape in ((1, 4, 2, 2), (3, 12, 5, 7), (2, 64, 5, 7)):
        assert _native._nhwc_grad_kind(_cl(*shape, dtype=dtype), _cl(*shape, dtype=dtype)) == KIND[dtype]


def test_other_pairs_keep_the_planar_route():
    kind = _native._nhwc_grad_kind
    src = _cl(2, 8, 5, 7)
    assert kind(src, torch.zeros(2, 8, 5, 7)) is None                                   # a planar upstream gradient
    assert kind(torch.zeros(2, 8, 5, 7), _cl(2, 8, 5, 7)) is None                       # a planar source
    assert kind(src, _cl(2, 8, 5, 7, torch.bfloat16)) is None                           # mismatched dtypes
    assert kind(_cl(2, 8, 5, 7, torch.float16), _cl(2, 8, 5, 7, torch.bfloat16)) is None
    assert kind(src, _cl(2, 8, 5, 7, torch.float64)) is None
    assert kind(_cl(1, 8, 5, 7), _cl(2, 8, 5, 7)) is None                               # a source broadcast over the batch
    assert kind(src, _cl(2, 8, 5, 6)) is None
    assert kind(_cl(2, 6, 5, 7), _cl(2, 6, 5, 7)) is None                               # C = 6
    sl = _cl(2, 12, 5, 7)[:, 4:]                                                        # a channel-sliced view
    assert sl.shape == src.shape and kind(src, sl) is None and kind(sl, src) is None
    assert kind(src, _cl(2, 8, 10, 7)[:, :, ::2]) is None                               # a row-strided view


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=str)
def test_a_misaligned_storage_offset_of_the_gradient_keeps_the_planar_route(dtype):
    n, c, h, w = 2, 8, 5, 7
    size, vec = torch.zeros((), dtype=dtype).element_size(), (16 if dtype == torch.float32 else 8)
    buf = torch.zeros(n * c * h * w + 16, dtype=dtype)
    assert buf.data_ptr() % 64 == 0
    src = _cl(n, c, h, w, dtype)
    for off in range(0, 9):
        g = torch.as_strided(buf, (n, c, h, w), (h * w * c, 1, w * c, c), off)
        assert g.is_contiguous(memory_format=CL) and not g.is_contiguous()
        aligned = (off * size) % vec == 0
        assert _native._nhwc_grad_kind(src, g) == (KIND[dtype] if aligned else None), (dtype, off)
        assert _native._nhwc_grad_kind(g, src) == (KIND[dtype] if aligned else None), (dtype, off)


def test_the_host_route_declines_cpu_tensors():
    flow = torch.zeros(2, 2, 5, 7)
    src, g = _cl(2, 8, 5, 7), _cl(2, 8, 5, 7)
    for ws, wf in ((True, True), (True, False), (False, True)):
        assert _native.warp_bwd_grad_nhwc(flow, src, g, flow_sign=1.0, g_scale=1.0, want_src=ws, want_flow=wf) is None
