"""CPU tier: ofl_warp_bwd_x16 (the backward warp of planes stored in fp16 / bf16) is declared, exported and rejects bad arguments
before touching a GPU -- in the style of test_cabi.py, which holds header and library to each other; this file names the symbol."""
import ctypes
import os
import re

from oflibpytorch_amd import _build, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_x16_warp():
    header = open(os.path.join(ROOT, 'include', 'oflib_hip.h')).read()
    assert re.search(r'^int ofl_warp_bwd_x16\(', header, flags=re.M)
    assert re.search(r'^#define OFL_X16_HALF 0$', header, flags=re.M) and re.search(r'^#define OFL_X16_BFLOAT 1$', header, flags=re.M)
    assert "ofl_warp_bwd_x16" in _native.exported_symbols()
    assert hasattr(ctypes.CDLL(_build.build()), "ofl_warp_bwd_x16")
    assert os.path.join("csrc", "ofl_warp_half.hip") in " ".join(_build.SOURCES)


def _call(lib, *, flow=16, src=16, dst=16, src_b=0, addend=0, flow_flags=0, src_flags=0, dst_flags=0, n=1, c=1, h=8, w=8,
          flow_sign=1.0, round_mode=0, dtype=1):
    p = ctypes.c_void_p          # (pointers are never dereferenced: every call here is rejected before a launch)
    return lib.ofl_warp_bwd_x16(p(flow), 0, flow_sign, p(src), 0, p(src_b), 0, p(0), 0, p(0), 0, p(addend), 0, 1.0, 1.0, p(dst), p(0),
                                p(flow_flags), p(src_flags), p(dst_flags), n, c, h, w, round_mode, dtype, p(0))


def test_x16_warp_rejects_bad_arguments_without_a_gpu():
    lib = _native.load_library()
    # NULL required pointers
    assert _call(lib, flow=0) == -1 and _call(lib, src=0) == -1 and _call(lib, dst=0) == -1
    # shapes
    assert _call(lib, c=0) == -2 and _call(lib, n=0) == -2 and _call(lib, h=0) == -2 and _call(lib, w=-1) == -2
    # dtype: 0 = fp16, 1 = bf16, nothing else; flow_sign +-1; round mode 0..2
    assert _call(lib, dtype=2) == -3 and _call(lib, dtype=-1) == -3
    assert _call(lib, flow_sign=0.5) == -3 and _call(lib, round_mode=3) == -3
    # what the 16-bit kernels do not take is declined (-4), for the caller to convert and call ofl_warp_bwd_f32
    for dt in (0, 1):
        assert _call(lib, dtype=dt, src_b=16) == -4 and _call(lib, dtype=dt, addend=16) == -4
        assert _call(lib, dtype=dt, flow_flags=16) == -4 and _call(lib, dtype=dt, src_flags=16, flow_flags=16) == -4
        assert _call(lib, dtype=dt, dst_flags=16) == -4
        assert _call(lib, dtype=dt, round_mode=1) == -4 and _call(lib, dtype=dt, round_mode=2) == -4
        assert _call(lib, dtype=dt, w=3) == -4 and _call(lib, dtype=dt, h=1) == -4          # beyond the staged kernels
        assert _call(lib, dtype=dt, h=4096, w=4096) == -4                                       # H * W >= 2^24
    # off the automatic warp path the fp32 kernels are the ones under test
    assert lib.ofl_set_option(1, 1) == 0
    try:
        assert _call(lib) == -4
    finally:
        assert lib.ofl_set_option(1, 0) == 0


def test_host_routes_only_device_tensors_of_16_bits_to_the_x16_warp():
    import torch
    flow = torch.zeros(1, 2, 8, 8)
    for dt in (torch.float16, torch.bfloat16):
        assert _native._warp_bwd_x16(flow, torch.zeros(1, 3, 8, 8, dtype=dt)) is None              # a CPU tensor: the present route
    assert _native._warp_bwd_x16(flow, torch.zeros(1, 3, 8, 8)) is None                            # fp32
    assert _native._X16_DTYPES == {torch.float16: 0, torch.bfloat16: 1}
