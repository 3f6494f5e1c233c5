"""CPU tier of the dirty-memory tests: the harness itself (tests/dirty_memory.py) on CPU tensors, the inventory of `_native.py`'s
allocation sites against the case table of tests/test_gpu_dirty_memory.py, and that table's atomic-exception list.  No device."""
import ast
import os
import re

import pytest
import torch

import dirty_memory as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [((3, 5), torch.float32, None), ((2, 3, 4, 5), torch.float16, torch.channels_last), ((7,), torch.int32, None),
          ((2, 4, 3), torch.bool, None), ((1, 16), torch.float64, None), ((2, 1, 3, 3), torch.uint8, torch.channels_last),
          ((0, 3), torch.float32, None), ((5, 0, 2), torch.int64, None)]


def _allocate(h, fn, shape, dtype, fmt, device='cpu'):
    """One allocation through the proxy, from a function whose name the log must show."""
    def some_primitive():
        kw = {} if fmt is None else {"memory_format": fmt}
        return getattr(h.proxy, fn)(shape, dtype=dtype, device=device, **kw)
    return some_primitive()


@pytest.fixture
def harness():
    return dm.Harness


@pytest.mark.parametrize("fill", dm.FILLS)
def test_canary_is_position_dependent_and_avoids_the_trivial_bytes(fill):
    c = dm.canary(dm.GUARD, fill)
    assert c.dtype == torch.uint8 and c.numel() == dm.GUARD
    for bad in (0x00, 0xFF, fill):
        assert not bool((c == bad).any())
    assert len(set(c.tolist())) > 200                        # not constant: nearly every byte value occurs
    assert not torch.equal(c[:-1], c[1:])
    assert not torch.equal(dm.canary(dm.GUARD, fill, 1), c)


@pytest.mark.parametrize("fill", dm.FILLS)
@pytest.mark.parametrize("shape,dtype,fmt", SHAPES, ids=str)
def test_body_fill_guards_shape_and_strides(harness, fill, shape, dtype, fmt):
    h = harness(fill)
    t = _allocate(h, "empty", shape, dtype, fmt)
    real = torch.empty(shape, dtype=dtype) if fmt is None else torch.empty(shape, dtype=dtype, memory_format=fmt)
    assert t.shape == real.shape and t.dtype == real.dtype and t.stride() == real.stride() and t.device == real.device
    for f in (torch.contiguous_format, torch.channels_last) if t.dim() == 4 else (torch.contiguous_format,):
        assert t.is_contiguous(memory_format=f) == real.is_contiguous(memory_format=f)
    assert len(h.log) == 1
    caller, lshape, ldtype, lfill, buf = h.log[0]
    assert caller == "some_primitive" and tuple(lshape) == tuple(shape) and ldtype == dtype and lfill == fill
    nbytes = real.numel() * real.element_size()
    assert buf.dtype == torch.uint8 and buf.numel() == 2 * dm.GUARD + nbytes and dm.GUARD % 512 == 0
    assert nbytes == 0 or t.data_ptr() == buf.data_ptr() + dm.GUARD        # the body starts one guard in: the allocation's alignment is kept
    assert bool((buf[dm.GUARD:dm.GUARD + nbytes] == fill).all())
    assert torch.equal(dm.as_bytes(t), torch.full((nbytes,), fill, dtype=torch.uint8))
    assert torch.equal(buf[:dm.GUARD], dm.canary(dm.GUARD, fill)) and not bool((buf[dm.GUARD + nbytes:] == fill).any())
    h.check_guards()
    # a write to every element of the tensor stays inside the body
    t.copy_(torch.ones(shape).to(dtype))
    h.check_guards()


@pytest.mark.parametrize("fill", dm.FILLS)
def test_zeros_bodies_are_zero_under_every_fill(harness, fill):
    h = harness(fill)
    for shape, dtype, fmt in SHAPES:
        t = _allocate(h, "zeros", shape, dtype, None)
        assert not bool(dm.as_bytes(t).any())
        assert t.shape == torch.Size(shape) and t.dtype == dtype
    h.check_guards()
    assert [a.zeros for a in h.log] == [True] * len(SHAPES)


def test_the_proxy_takes_shapes_as_torch_does_and_forwards_everything_else(harness):
    h = harness(0x55)
    p = h.proxy
    assert p.empty(2, 3, dtype=torch.int32).shape == (2, 3) and p.empty((2, 3), dtype=torch.int32).shape == (2, 3)
    assert p.zeros(4, dtype=torch.int32, device=torch.device('cpu')).tolist() == [0] * 4
    assert p.empty(3).dtype == torch.get_default_dtype()
    assert p.float32 is torch.float32 and p.cuda is torch.cuda and p.Tensor is torch.Tensor and p.channels_last is torch.channels_last
    assert p.empty is not torch.empty and torch.empty.__module__ != dm.__name__      # torch.empty itself is not patched
    with pytest.raises(AttributeError):
        p.empty_like = None


@pytest.mark.parametrize("side,offset", [("before", -1), ("after", 0), ("before", -dm.GUARD), ("after", dm.GUARD - 1)])
def test_a_byte_outside_the_body_fails_the_guard_check_and_names_the_side(harness, side, offset):
    h = harness(0xFF)
    _allocate(h, "empty", (4, 4), torch.float32, None)
    t = _allocate(h, "empty", (3, 5), torch.float32, None)
    _allocate(h, "zeros", (2,), torch.int32, None)
    h.check_guards()
    buf, nbytes = h.log[1].buffer, 60
    at = dm.GUARD + (offset if side == "before" else nbytes + offset)
    buf[at] = buf[at] ^ 0x01                                 # one bit of one byte, through the base buffer
    with pytest.raises(AssertionError) as err:
        h.check_guards()
    msg = str(err.value)
    assert "allocation 1" in msg and "(3, 5)" in msg and "some_primitive" in msg and ("written %s its body" % side) in msg
    assert ("first at offset %d, last at %d" % (offset, offset)) in msg
    t.fill_(1.0)                                             # the body itself is free to change
    buf[at] = buf[at] ^ 0x01
    h.check_guards()


def test_a_run_of_stray_zeros_or_nans_cannot_pass_for_the_canary(harness):
    for fill, stray in ((0x00, 0x00), (0xFF, 0xFF), (0x55, 0x55), (0x55, 0x00)):
        h = harness(fill)
        _allocate(h, "empty", (8,), torch.float32, None)
        h.log[0].buffer[dm.GUARD + 32: dm.GUARD + 48] = stray        # a 16-byte store past the end
        with pytest.raises(AssertionError, match="written after its body: 16 bytes differ, first at offset 0, last at 15"):
            h.check_guards()


@pytest.mark.parametrize("fill", dm.FILLS)
def test_guarded_inputs(harness, fill):
    h = harness(fill)
    g = torch.Generator().manual_seed(1)
    a = torch.randn(2, 3, 4, 5, generator=g)
    cl = a.contiguous(memory_format=torch.channels_last)
    m = torch.rand(2, 4, 5, generator=g) > 0.5
    ga, gcl, gm = h.guarded(a, "a"), h.guarded(cl, "cl"), h.guarded(m, "m")
    assert torch.equal(ga, a) and ga.stride() == a.stride() and ga.data_ptr() != a.data_ptr()
    assert torch.equal(gcl, cl) and gcl.stride() == cl.stride() and gcl.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(gm, m) and gm.dtype == torch.bool
    for name, buf, nbytes, saved in h.inputs:                # both guards of an input hold the fill byte
        assert bool((buf[:dm.GUARD] == fill).all()) and bool((buf[dm.GUARD + nbytes:] == fill).all())
    assert not h.log                                         # inputs are no allocations of the code under test
    # None and broadcast inputs pass through unchanged
    one = torch.randn(1, 2, 4, 5, generator=g)
    ex = one.expand(3, -1, -1, -1)
    assert h.guarded(None) is None and h.guarded(ex) is ex and len(h.inputs) == 3
    h.check_inputs_unchanged()
    gm[1, 2, 3] = not bool(gm[1, 2, 3])
    with pytest.raises(AssertionError, match=r"m \(40 bytes\) or its guards were written: 1 bytes differ, first at offset 33, last at 33"):
        h.check_inputs_unchanged()
    gm[1, 2, 3] = not bool(gm[1, 2, 3])
    h.check_inputs_unchanged()
    h.inputs[0][1][dm.GUARD - 2] ^= 0x10                     # a write just in front of an input
    with pytest.raises(AssertionError, match=r"a \(480 bytes\) or its guards were written: 1 bytes differ, first at offset -2"):
        h.check_inputs_unchanged()


def test_the_context_manager_replaces_torch_in_native_only_and_restores_it():
    from oflibpytorch_amd import _autograd, _native, flow_class
    assert _native.torch is torch and _autograd.torch is torch
    h = dm.Harness(0x55)
    with h:
        assert isinstance(_native.torch, dm._TorchProxy) and isinstance(_autograd.torch, dm._TorchProxy)
        assert flow_class.torch is torch and torch.empty is dm.torch.empty
        x = _native.torch.zeros(3, dtype=torch.int32)
        assert _native.torch.float16 is torch.float16 and _native.torch.is_grad_enabled() is torch.is_grad_enabled()
    assert _native.torch is torch and _autograd.torch is torch
    assert x.tolist() == [0, 0, 0] and len(h.log) == 1 and h.log[0].caller == "test_the_context_manager_replaces_torch_in_native_only_and_restores_it"
    with pytest.raises(ZeroDivisionError):
        with dm.Harness(0x00):
            1 / 0
    assert _native.torch is torch and _autograd.torch is torch           # restored after an exception too


def test_same_bits_comparison_counts_nan_payloads_and_bool_bytes():
    a = torch.tensor([1.0, float('nan'), -0.0])
    b = a.clone()
    dm.assert_same_bits((a, None), (b, None), "x")
    b.view(torch.int32)[1] ^= 1                              # another NaN: equal as numbers with equal_nan, not as bits
    with pytest.raises(AssertionError, match="differs in 1 bytes, elements 1 ... 1"):
        dm.assert_same_bits(a, b, "x")
    with pytest.raises(AssertionError):
        dm.assert_same_bits(a, torch.tensor([1.0, float('nan'), 0.0]), "x")
    raw = torch.tensor([0, 1, 2, 255], dtype=torch.uint8)
    with pytest.raises(AssertionError, match="neither 0 nor 1"):
        dm.assert_bool_bytes((a, raw.view(torch.bool)), "x")
    dm.assert_bool_bytes((a, raw[:2].view(torch.bool), None), "x")


# ---- inventory ---------------------------------------------------------------------------------------------------------------------
def _allocating_functions():
    """{function name: [line numbers]} of the functions of _native.py whose body calls torch.empty / torch.zeros / *.empty_like /
    *.new_empty (NumPy's host arrays are not device memory)."""
    with open(os.path.join(ROOT, 'oflibpytorch_amd', '_native.py')) as fh:
        tree = ast.parse(fh.read())
    out = {}

    def visit(node, owner):
        for child in ast.iter_child_nodes(node):
            name = child.name if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)) else owner
            if isinstance(child, ast.Call) and isinstance(child.func, ast.Attribute):
                f = child.func
                base = f.value.id if isinstance(f.value, ast.Name) else None
                if (f.attr in ("empty", "zeros") and base == "torch") or (f.attr in ("empty_like", "new_empty", "zeros_like", "new_zeros") and base not in ("np", "numpy")):
                    out.setdefault(owner, []).append(child.lineno)
            visit(child, name)

    visit(tree, "<module>")
    return out


def test_every_allocation_site_of_native_has_a_dirty_memory_case():
    import test_gpu_dirty_memory as table                    # (builds the case table; touches no device)
    sites = _allocating_functions()
    assert "<module>" not in sites
    assert sum(len(v) for v in sites.values()) >= 85 and {"_splat_fwd_raw", "_fallback_accum", "flow_extents", "splat_grad", "_mesh_plan",
                                                          "_new_host_slot", "decode_flo"} <= set(sites)
    covered = set()
    for c in table.CASES:
        covered |= {c.primitive} if isinstance(c.primitive, str) else set()
        covered |= set(c.callees)
    assert covered <= set(sites), "cases name functions that allocate nothing: %s" % sorted(covered - set(sites))
    uncovered = {k: v for k, v in sites.items() if k not in covered}
    assert not uncovered, "allocation sites of _native.py without a dirty-memory case (function: lines): %s" % uncovered


def test_the_case_table_is_well_formed():
    import test_gpu_dirty_memory as table
    ids = [c.id for c in table.CASES]
    assert len(set(ids)) == len(ids) and len(ids) > 200
    for c in table.CASES:
        assert c.control is not None or c.atomic is not None, "%s has neither a control nor a bar" % c.id
        assert callable(c.build) and callable(c.run)
    import test_gpu_warp_kernel_choice as wk
    ran = {wk.RECORDED[c.id[len("warp.choice."):]] for c in table.CASES if c.id.startswith("warp.choice.")}
    assert ran == set(wk.RECORDED.values())                  # one case per distinct recorded kernel name


def test_every_atomic_exception_names_a_case_and_a_line():
    import test_gpu_dirty_memory as table
    listed = table.ATOMIC_EXCEPTIONS
    atomic = [c.id for c in table.CASES if c.atomic is not None]
    for prefix, (kernel, where) in listed.items():
        assert any(i.startswith(prefix) for i in atomic), "no case with an atomic bar is named %s*" % prefix
        m = re.fullmatch(r"(ofl_\w+\.hip):(\d+)", where)
        assert m, where
        with open(os.path.join(ROOT, 'oflibpytorch_amd', 'csrc', m.group(1))) as fh:
            line = fh.read().split("\n")[int(m.group(2)) - 1]
        assert "atomicAdd(" in line, "%s: no atomicAdd on that line: %s" % (where, line.strip())
        assert prefix in table.__doc__ and where in table.__doc__ and kernel.split("<")[0] in table.__doc__
    for i in atomic:                                         # and the list does not grow silently
        assert any(i.startswith(p) for p in listed), "%s has an atomic bar but is not on the exception list" % i
