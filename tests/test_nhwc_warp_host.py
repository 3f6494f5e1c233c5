"""CPU tier of the channels_last warp (ofl_warp_bwd_nhwc): the routing predicate `_native._nhwc_kind` on CPU tensors --
what qualifies for the N-H-W-C kernel and what keeps the planar route -- and the entry point in the header and the built library."""
import os
import re

import pytest
import torch

from oflibpytorch_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CL = torch.channels_last
KIND = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}          # OFL_X16_HALF, OFL_X16_BFLOAT, OFL_NHWC_F32
VEC_BYTES = {torch.float16: 8, torch.bfloat16: 8, torch.float32: 16}    # a lane's vector


def _cl(n, c, h, w, dtype=torch.float32):
    t = torch.zeros(n, c, h, w, dtype=dtype).contiguous(memory_format=CL)
    assert t.data_ptr() % 64 == 0
    return t


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("c", [4, 12, 64])
def test_channels_last_float_tensors_qualify(c, dtype):
    for shape in ((1, c, 2, 2), (3, c, 5, 7)):
        assert _native._nhwc_kind(_cl(*shape, dtype=dtype)) == KIND[dtype]


def test_header_constants_match_the_binding():
    text = open(os.path.join(ROOT, "include", "oflib_hip.h")).read()
    for name, val in (("OFL_X16_HALF", 0), ("OFL_X16_BFLOAT", 1), ("OFL_NHWC_F32", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), text), name


def test_other_tensors_keep_the_planar_route():
    kind = _native._nhwc_kind
    assert kind(torch.zeros(2, 8, 5, 7)) is None                                        # N-C-H-W contiguous
    assert kind(_cl(2, 1, 5, 7)) is None                                                # C = 1: the two formats coincide
    assert kind(_cl(2, 8, 1, 1)) is None                                                # a 1 x 1 frame: they coincide too
    assert kind(_cl(2, 6, 5, 7)) is None                                                # C = 6
    assert kind(_cl(2, 2, 5, 7)) is None
    assert kind(_cl(2, 8, 5, 7, torch.uint8)) is None
    assert kind(_cl(2, 8, 5, 7, torch.float64)) is None
    assert kind(_cl(2, 8, 5, 7, torch.int32)) is None
    assert kind(torch.zeros(8, 5, 7)) is None                                           # 3-D
    assert kind(torch.zeros(5, 7, 8).permute(2, 0, 1)) is None                          # 3-D, channels innermost
    assert kind(_cl(2, 8, 1, 7)) is None and kind(_cl(2, 8, 5, 1)) is None              # H or W below 2
    sl = _cl(2, 12, 5, 7)[:, 4:]                                                        # a channel slice: pixels 12 elements apart, 8 used
    assert sl.shape[1] == 8 and not sl.is_contiguous(memory_format=CL) and kind(sl) is None
    assert kind(_cl(2, 8, 5, 7)[:, :, ::2]) is None                                     # a row-strided view


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=str)
def test_a_storage_offset_that_breaks_the_vector_alignment_keeps_the_planar_route(dtype):
    n, c, h, w = 2, 8, 5, 7
    size, vec = torch.zeros((), dtype=dtype).element_size(), VEC_BYTES[dtype]
    buf = torch.zeros(n * c * h * w + 16, dtype=dtype)
    assert buf.data_ptr() % 64 == 0
    for off in range(0, 9):
        t = torch.as_strided(buf, (n, c, h, w), (h * w * c, 1, w * c, c), off)
        assert t.is_contiguous(memory_format=CL) and not t.is_contiguous()
        aligned = (off * size) % vec == 0
        assert (_native._nhwc_kind(t) == KIND[dtype]) if aligned else (_native._nhwc_kind(t) is None), (dtype, off)
    # fp32 at 1 or 2 elements, 16-bit at 1 to 3 elements: all declined (the loop above, spelled out)
    bad = (1, 2) if dtype == torch.float32 else (1, 2, 3)
    for off in bad:
        assert _native._nhwc_kind(torch.as_strided(buf, (n, c, h, w), (h * w * c, 1, w * c, c), off)) is None


def test_host_route_declines_cpu_tensors_and_non_plain_calls():
    flow = torch.zeros(2, 2, 5, 7)
    t = _cl(2, 8, 5, 7)
    assert _native.warp_bwd_nhwc(flow, t) is None                                       # a CPU tensor: staged by the planar route
    assert _native._warp_bwd_nhwc(flow, t) is None
    assert _native.warp_bwd_nhwc(flow, torch.zeros(2, 8, 5, 7)) is None
    assert _native.NHWC_MIN_CHANNELS >= 4 and _native.NHWC_MIN_CHANNELS % 4 == 0


def test_header_declares_the_entry_point_and_the_library_exports_it():
    text = open(os.path.join(ROOT, "include", "oflib_hip.h")).read()
    m = re.search(r"\bint\s+ofl_warp_bwd_nhwc\s*\(([^;]*)\)\s*;", text)
    assert m, "include/oflib_hip.h does not declare ofl_warp_bwd_nhwc"
    args = [a.strip().split()[-1].lstrip("*") for a in m.group(1).replace("\n", " ").split(",")]
    assert args == ["flow", "flow_bs", "flow_sign", "src", "src_bs", "src_mask", "src_mask_bs", "flow_mask", "flow_mask_bs",
                    "dst", "valid", "n", "c", "h", "w", "dtype", "stream"]
    assert "ofl_warp_bwd_nhwc" in _native.exported_symbols()
    lib = _native.load_library()
    assert hasattr(lib, "ofl_warp_bwd_nhwc") and len(lib.ofl_warp_bwd_nhwc.argtypes) == len(args)


def test_entry_point_rejects_and_declines_without_a_device():
    """Argument checks come before any launch, so they run without a GPU: pointers are only compared, never followed."""
    import ctypes
    lib = _native.load_library()
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 63) & ~63
    P = ctypes.c_void_p

    def call(n=2, c=8, h=5, w=7, dtype=2, src=base, dst=base + 2048, flow_bs=70, src_bs=280, flow_sign=1.0, flow=base):
        return lib.ofl_warp_bwd_nhwc(P(flow), flow_bs, flow_sign, P(src), src_bs, None, 0, None, 0, P(dst), None, n, c, h, w, dtype, None)
    E_NULL, E_SHAPE, E_ARG, E_UNSUPPORTED = -1, -2, -3, -4
    assert call(flow=None) == E_NULL and call(src=None) == E_NULL and call(dst=None) == E_NULL
    assert call(dtype=3) == E_ARG and call(dtype=-1) == E_ARG
    assert call(flow_bs=-1) == E_ARG and call(src_bs=-1) == E_ARG and call(n=-1) == E_ARG and call(c=-4) == E_ARG
    assert call(flow_sign=0.5) == E_ARG
    assert call(n=0) == E_SHAPE
    for kw in (dict(c=6), dict(c=2), dict(c=3), dict(h=1), dict(w=1)):
        assert call(**kw) == E_UNSUPPORTED, kw
    for dtype, offs in ((2, (4, 8, 12)), (0, (2, 4, 6)), (1, (2, 4, 6))):
        for o in offs:
            assert call(dtype=dtype, src=base + o) == E_UNSUPPORTED and call(dtype=dtype, dst=base + 2048 + o) == E_UNSUPPORTED
