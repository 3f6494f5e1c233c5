"""CPU tier: the backward pass of the 16-bit warp (ofl_warp_bwd_grad_x16, ofl_splat_sum_x16) is declared, exported and rejects bad
arguments before touching a GPU, and `WarpFn.backward` hands `_native.warp_bwd_grad_x16` exactly the calls it is meant for -- a 16-bit
source on the device, an upstream gradient of the same dtype, no `src_b`, no batch broadcast -- and keeps the present route otherwise
and when the call is declined."""
import ctypes
import os
import re

import pytest
import torch

from oflibpytorch_amd import _autograd, _build, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ofl_warp_bwd_grad_x16", "ofl_splat_sum_x16")


def test_header_declares_and_library_exports_the_two_entry_points():
    header = open(os.path.join(ROOT, 'include', 'oflib_hip.h')).read()
    lib = ctypes.CDLL(_build.build())
    for name in NAMES:
        assert re.search(r'^int %s\(' % name, header, flags=re.M)
        assert name in _native.exported_symbols() and hasattr(lib, name)
    assert _native.ABI_VERSION == 36 and _native.load_library().ofl_version() == 36


def _grad(lib, *, flow=16, src=16, gout=16, gflow=16, flow_bs=0, src_bs=0, n=1, c=1, h=8, w=8, flow_sign=1.0, dtype=1):
    p = ctypes.c_void_p          # (pointers are never dereferenced: every call here is rejected before a launch)
    return lib.ofl_warp_bwd_grad_x16(p(flow), flow_bs, flow_sign, p(src), src_bs, p(gout), 1.0, p(gflow), n, c, h, w, dtype, p(0))


def _sum(lib, *, flow=16, data=16, dst=16, ws=16, accum=16, flow_bs=0, data_bs=0, n=1, c=1, h=8, w=8, flow_sign=1.0, dtype=1):
    p = ctypes.c_void_p
    return lib.ofl_splat_sum_x16(p(flow), flow_bs, flow_sign, p(data), data_bs, 1.0, p(dst), p(ws), 1 << 30, p(accum), n, c, h, w, dtype, p(0))


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _native.load_library()
    # NULL required pointers
    assert _grad(lib, flow=0) == -1 and _grad(lib, src=0) == -1 and _grad(lib, gout=0) == -1 and _grad(lib, gflow=0) == -1
    assert _sum(lib, flow=0) == -1 and _sum(lib, data=0) == -1 and _sum(lib, dst=0) == -1 and _sum(lib, ws=0) == -1 and _sum(lib, accum=0) == -1
    for call in (_grad, _sum):
        # dtype: 0 = fp16, 1 = bf16, nothing else; flow_sign +-1; no negative batch strides; at least one plane
        assert call(lib, dtype=2) == -3 and call(lib, dtype=-1) == -3
        assert call(lib, flow_sign=0.5) == -3 and call(lib, flow_sign=0.0) == -3
        assert call(lib, flow_bs=-128) == -3
        assert call(lib, c=0) == -2 and call(lib, c=-1) == -2 and call(lib, n=0) == -2 and call(lib, h=0) == -2 and call(lib, w=-1) == -2
    assert _grad(lib, src_bs=-64) == -3 and _sum(lib, data_bs=-64) == -3
    assert _grad(lib, src=17) == -3 and _grad(lib, gout=17) == -3 and _sum(lib, data=17) == -3 and _sum(lib, dst=17) == -3   # 2-byte alignment
    # frames the kernels do not take are declined (-4) and nothing is launched: the caller converts and calls the fp32 entry points
    for dt in (0, 1):
        assert _grad(lib, dtype=dt, w=3) == -4 and _grad(lib, dtype=dt, w=2) == -4 and _grad(lib, dtype=dt, h=1) == -4
        assert _grad(lib, dtype=dt, h=4096, w=4096) == -4
        assert _sum(lib, dtype=dt, w=3) == -4
    assert lib.ofl_set_option(1, 1) == 0          # off the automatic warp path the fp32 kernels are the ones under test
    try:
        assert _grad(lib) == -4
    finally:
        assert lib.ofl_set_option(1, 0) == 0


def test_host_binding_declines_what_is_not_a_16_bit_device_call():
    flow = torch.zeros(2, 2, 8, 8)
    for dt in (torch.float16, torch.bfloat16):
        x = torch.zeros(2, 3, 8, 8, dtype=dt)
        assert _native.warp_bwd_grad_x16(flow, x, x) is None                        # CPU tensors
    x = torch.zeros(2, 3, 8, 8)
    assert _native.warp_bwd_grad_x16(flow, x, x) is None                            # fp32


# ---- WarpFn.backward's dispatch, on stand-ins: a tensor that SAYS it lives on the HIP device, a ctx with what backward reads ----
class _OnDevice(torch.Tensor):
    @property
    def device(self):
        return torch.device('cuda', 0)


class _Ctx:
    def __init__(self, flow, src, src_b=None, addend_meta=None, needs=(True, True, False, False)):
        self.saved_tensors = (flow, src, src_b)
        self.signs = (1.0, 1.0, 1.0)
        self.addend_meta = addend_meta
        self.needs_input_grad = needs + (False,)


def _on_device(t):
    return t.as_subclass(_OnDevice)


@pytest.fixture
def routes(monkeypatch):
    """The two routes as recorders: `calls` lists what each was given; the fp32 route answers with recognisable tensors."""
    calls = {"x16": [], "f32": []}

    def f32(flow, src, g, **kw):
        calls["f32"].append((src, g, kw))
        return torch.full(src.shape, 2.0), torch.full((g.shape[0], 2) + tuple(g.shape[2:]), 3.0)
    monkeypatch.setattr(_native, "warp_bwd_grad", f32)
    monkeypatch.setattr(_autograd, "_reduce_to", lambda g, like: g)                 # (no device to move to in this tier)
    return calls


def _backward(ctx, g):
    with torch.no_grad():
        return _autograd.WarpFn.backward(ctx, g)


def test_backward_never_offers_the_other_calls_to_the_16_bit_route(routes, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("warp_bwd_grad_x16 was called")
    monkeypatch.setattr(_native, "warp_bwd_grad_x16", boom)
    flow = torch.zeros(3, 2, 8, 8)
    bf = lambda *s: torch.ones(*s).to(torch.bfloat16)
    cases = [(_Ctx(flow, _on_device(torch.ones(3, 4, 8, 8))), torch.ones(3, 4, 8, 8)),             # an fp32 source on the device
             (_Ctx(flow, bf(3, 4, 8, 8)), bf(3, 4, 8, 8)),                                         # a 16-bit CPU tensor
             (_Ctx(flow, _on_device(bf(3, 2, 8, 8)), src_b=bf(3, 2, 8, 8)), bf(3, 2, 8, 8)),       # src_b
             (_Ctx(flow, _on_device(bf(1, 4, 8, 8))), bf(3, 4, 8, 8)),                             # a source broadcast over the batch
             (_Ctx(flow, _on_device(bf(3, 4, 8, 8))), torch.ones(3, 4, 8, 8)),                     # an fp32 upstream gradient
             (_Ctx(flow, _on_device(bf(3, 4, 8, 8))), bf(3, 4, 8, 8).to(memory_format=torch.channels_last))]
    for i, (ctx, g) in enumerate(cases):
        out = _backward(ctx, g)
        assert len(routes["f32"]) == i + 1 and out[0] is not None and out[1] is not None
        assert routes["f32"][-1][0].dtype == torch.float32 and routes["f32"][-1][1].is_contiguous()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=str)
def test_a_declined_16_bit_call_gives_what_the_present_route_gives(routes, monkeypatch, dtype):
    def declined(flow, src, g, **kw):
        routes["x16"].append((src, g, kw))
        return None
    monkeypatch.setattr(_native, "warp_bwd_grad_x16", declined)
    flow = torch.zeros(2, 2, 8, 8)
    src = _on_device((torch.arange(2 * 3 * 8 * 8).reshape(2, 3, 8, 8) % 13).to(dtype))
    g = torch.ones(2, 3, 8, 8).to(dtype)
    out = _backward(_Ctx(flow, src), g)
    # offered once, with the 16-bit tensors themselves and both gradients wanted ...
    assert len(routes["x16"]) == 1
    s16, g16, kw = routes["x16"][0]
    assert s16 is src and g16.dtype == dtype and kw == dict(flow_sign=1.0, g_scale=1.0, want_src=True, want_flow=True)
    # ... then the present route, unchanged: the up-converted source, the same upstream gradient, its results handed on
    assert len(routes["f32"]) == 1
    s32, g32, kw = routes["f32"][0]
    assert s32.dtype == torch.float32 and torch.equal(s32, src.float()) and g32 is g
    assert kw == dict(flow_sign=1.0, g_scale=1.0, want_src=True, want_flow=True)
    assert torch.equal(out[0], torch.full((2, 2, 8, 8), 3.0)) and torch.equal(out[1], torch.full((2, 3, 8, 8), 2.0))
    assert out[2:] == (None, None, None)


def test_an_accepted_16_bit_call_is_the_whole_backward(routes, monkeypatch):
    gs, gf = torch.full((2, 3, 8, 8), 5.0).to(torch.bfloat16), torch.full((2, 2, 8, 8), 7.0)
    monkeypatch.setattr(_native, "warp_bwd_grad_x16", lambda flow, src, g, **kw: (gs if kw["want_src"] else None, gf if kw["want_flow"] else None))
    flow, src = torch.zeros(2, 2, 8, 8), _on_device(torch.ones(2, 3, 8, 8).to(torch.bfloat16))
    out = _backward(_Ctx(flow, src), torch.ones(2, 3, 8, 8).to(torch.bfloat16))
    assert out[0] is gf and out[1] is gs and out[2:] == (None, None, None) and not routes["f32"]
    out = _backward(_Ctx(flow, src, needs=(False, True, False, False)), torch.ones(2, 3, 8, 8).to(torch.bfloat16))
    assert out[0] is None and out[1] is gs and not routes["f32"]
