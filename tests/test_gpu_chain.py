"""GPU tier of Flow.chain / chain_flows (ofl_chain.hip) against tests/chain_oracle.py: vectors and mask bytes bit for
bit, with no exceptions, and against the fold of combine_with(..., 3) on the device.

Frames: 2 x 2 (the smallest allowed), 5 x 7 and 8 x 12 (one partly filled block), 20 x 28 (three blocks; the planted pixels), 67 x 131 (35
blocks with a ragged tail), 1080 x 1920 (8100 blocks, offsets far beyond a block's pixels; the kernel has no block cap).  T in 2, 3, 5,
and 32 (the longest chain the kernel arguments hold) at 20 x 28.  The inputs and what they show are checked on the CPU
(tests/test_chain_host.py)."""
import ctypes

import numpy as np
import pytest
import torch

import chain_oracle as co

pytestmark = pytest.mark.gpu

REFS = ['s', 't']
TABLE = [(h, w, t) for h, w in co.FRAMES for t in (2, 3, 5)] + [(20, 28, 32)]
KERNEL = 'flow_chain_kernel'


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _objs(flows, masks, ref, half=()):
    import oflibpytorch_amd as ofl
    out = []
    for k, (f, m) in enumerate(zip(flows, masks)):
        v = torch.from_numpy(np.array(f)).to(_dev())
        out.append(ofl.Flow(v.half() if k in half else v, ref, None if m is None else torch.from_numpy(np.array(m)).to(_dev())))
    return out


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.uint8) if a.dtype == bool else a.view(np.uint32)


def _same(flow, vecs, valid, what=""):
    assert flow.vecs.dtype == torch.float32 and tuple(flow.vecs.shape) == vecs.shape, what
    assert np.array_equal(_bits(flow.vecs), _bits(vecs)), (what, "vectors")
    mask_bytes = _bits(flow.mask)
    assert set(np.unique(mask_bytes)) <= {0, 1}, (what, "mask bytes")
    assert np.array_equal(mask_bytes, _bits(valid)), (what, "mask")


def _same_flows(a, b, what=""):
    assert np.array_equal(_bits(a.vecs), _bits(b.vecs)), (what, "vectors")
    assert np.array_equal(_bits(a.mask), _bits(b.mask)), (what, "mask")


@pytest.mark.parametrize("return_all", [False, True])
@pytest.mark.parametrize("ref", REFS)
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("h,w,t", TABLE)
def test_kernel_is_the_oracle_bit_for_bit(h, w, t, n, ref, return_all):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _native
    flows, masks = co.case(n, h, w, ref, t)
    vecs, valid, _ = co.reference(n, h, w, ref, t)
    objs = _objs(flows, masks, ref)
    res = ofl.Flow.chain(objs, return_all=return_all)
    assert KERNEL in _native.last_kernel_name()
    name = _native.last_kernel_name()                         # (demangled, or mangled where no demangler is installed)
    assert any(s in name for s in (('<true>', 'ILb1E') if return_all else ('<false>', 'ILb0E'))), name
    full, single = (t - 1, 0) if ref == 's' else (0, t - 1)
    if not return_all:
        assert isinstance(res, ofl.Flow) and res.ref == ref and res.vecs.device == objs[0].vecs.device
        _same(res, vecs[full], valid[full])
        return
    assert isinstance(res, list) and len(res) == t and res[single] is objs[single]
    for k in range(t):                                        # every prefix ('s') / suffix ('t') is the oracle's
        assert res[k].ref == ref
        _same(res[k], vecs[k], valid[k], "entry %d" % k)


@pytest.mark.parametrize("ref", REFS)
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("h,w,t", TABLE)
def test_chain_is_the_fold_of_mode_3_on_the_device(h, w, t, n, ref):
    """fp32 storage: the same bits as T - 1 launches of combine_with(..., 3), which took none of its early exits (co.fold asserts it)."""
    import oflibpytorch_amd as ofl
    objs = _objs(*co.case(n, h, w, ref, t), ref)
    fold = co.fold(objs, ref)
    out = ofl.Flow.chain(objs, return_all=True)
    for k in range(t):
        _same_flows(out[k], fold[k], "entry %d" % k)


@pytest.mark.parametrize("ref", REFS)
def test_full_size_against_the_device_fold(ref):
    """1080 x 1920, N = 1, T = 3: 8100 blocks per image (the kernel has no block cap and no stride), pixel offsets far beyond one block."""
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _native
    objs = _objs(*co.case(1, 1080, 1920, ref, 3), ref)
    fold = co.fold(objs, ref)
    out = ofl.Flow.chain(objs, return_all=True)
    assert KERNEL in _native.last_kernel_name()
    for k in range(3):
        assert bool(torch.equal(out[k].vecs.view(torch.int32), fold[k].vecs.view(torch.int32))), k
        assert bool(torch.equal(out[k].mask, fold[k].mask)), k
    full = out[-1] if ref == 's' else out[0]
    share = float(full.mask.float().mean())
    print("valid share of the full chain: %.3f" % share)
    assert 0.25 < share < 1.0
    one = ofl.Flow.chain(objs)
    assert bool(torch.equal(one.vecs.view(torch.int32), full.vecs.view(torch.int32))) and bool(torch.equal(one.mask, full.mask))


@pytest.mark.parametrize("want_all", [False, True])
@pytest.mark.parametrize("ref", REFS)
def test_views_give_the_bits_of_contiguous_copies(ref, want_all):
    """One flow is a batch-strided view (`big[::2]`), one sits at an offset storage pointer (4-byte aligned only), one mask is a
    batch-strided view and one sits at an odd address."""
    from oflibpytorch_amd import _chain
    n, h, w, t = 2, 20, 28, 5
    flows, masks = co.case(n, h, w, ref, t)
    dev = _dev()
    vs = [torch.from_numpy(np.array(f)).to(dev) for f in flows]
    ms = [None if m is None else torch.from_numpy(np.array(m)).to(dev) for m in masks]
    sign = -1.0 if ref == 's' else 1.0
    want = _chain.flow_chain(vs, ms, sign, want_all)
    assert all(v.is_contiguous() for v in vs)
    vv, mm = list(vs), list(ms)
    big = torch.full((2 * n, 2, h, w), 7.0, device=dev)
    big[::2] = vs[1]
    vv[1] = big[::2]
    flat = torch.full((vs[3].numel() + 3,), 7.0, device=dev)
    flat[1:1 + vs[3].numel()] = vs[3].reshape(-1)
    vv[3] = flat[1:1 + vs[3].numel()].view(n, 2, h, w)
    assert vv[1].stride(0) == 4 * h * w and vv[3].data_ptr() % 16 == 4 and vv[3].storage_offset() == 1
    k_strided, k_odd = [k for k in range(t) if ms[k] is not None][:2]
    bigm = torch.ones((2 * n, h, w), dtype=torch.bool, device=dev)
    bigm[::2] = ms[k_strided]
    mm[k_strided] = bigm[::2]
    flatm = torch.ones((ms[k_odd].numel() + 3,), dtype=torch.bool, device=dev)
    flatm[1:1 + ms[k_odd].numel()] = ms[k_odd].reshape(-1)
    mm[k_odd] = flatm[1:1 + ms[k_odd].numel()].view(n, h, w)
    assert mm[k_odd].data_ptr() % 2 == 1
    got = _chain.flow_chain(vv, mm, sign, want_all)
    for g, w_ in zip(got, want):
        assert g.shape == w_.shape and np.array_equal(_bits(g), _bits(w_))
    vecs, valid, _ = co.reference(n, h, w, ref, t)
    full = t - 1 if ref == 's' else 0
    if not want_all:
        assert np.array_equal(_bits(got[0]), _bits(vecs[full])) and np.array_equal(_bits(got[1]), _bits(valid[full]))


@pytest.mark.parametrize("ref", REFS)
def test_fp16_stored_flows_against_the_oracle_on_the_up_converted_values(ref):
    """Two of five flows are stored in fp16 and read as they are: the oracle runs on their exactly up-converted values."""
    import oflibpytorch_amd as ofl
    n, h, w, t = 2, 20, 28, 5
    flows, masks = co.case(n, h, w, ref, t)
    half = (1, 3)
    rounded = [f.astype(np.float16) if k in half else f for k, f in enumerate(flows)]
    vecs, valid = co.chain(rounded, masks, ref)
    objs = _objs(flows, masks, ref, half=half)
    assert [o._fv.dtype for o in objs] == [torch.float16 if k in half else torch.float32 for k in range(t)]
    out = ofl.Flow.chain(objs, return_all=True)
    assert [o._fv.dtype for o in objs] == [torch.float16 if k in half else torch.float32 for k in range(t)]   # no fp32 copy was made
    single = 0 if ref == 's' else t - 1
    for k in range(t):
        if k != single:
            _same(out[k], vecs[k], valid[k], "entry %d" % k)
    # (the fp16 rounding matters: the fp32 inputs give other bits)
    assert not np.array_equal(_bits(vecs[t - 1 if ref == 's' else 0]), _bits(co.reference(n, h, w, ref, t)[0][t - 1 if ref == 's' else 0]))


@pytest.mark.parametrize("ref", REFS)
def test_a_zero_flow_follows_the_general_formula(ref):
    """One flow of the clip is all zero.  The chain samples it like any other flow: the vectors it adds are 0, and its mask and the
    frame still invalidate the walks whose taps they do not cover -- the oracle's value.  The fold of combine_with takes the early exit of
    the reference here (an operand that is all zero under its mask: the other operand is returned as it is), so its MASK keeps the
    pixels that the zero flow's holes and the frame's edge would have invalidated; its vectors are the same numbers (DESIGN.md 3.31,
    7)."""
    import oflibpytorch_amd as ofl
    n, h, w, t = 2, 20, 28, 3
    flows, masks = co.case(n, h, w, ref, t)
    zero_at = co.walk_order(t, ref)[1]                        # the second flow of the walk: it has a mask, with holes
    flows = [np.zeros_like(f) if k == zero_at else f for k, f in enumerate(flows)]
    assert masks[zero_at] is not None and not masks[zero_at].all()
    vecs, valid = co.chain(flows, masks, ref)
    objs = _objs(flows, masks, ref)
    out = ofl.Flow.chain(objs, return_all=True)
    single = 0 if ref == 's' else t - 1
    for k in range(t):
        if k != single:
            _same(out[k], vecs[k], valid[k], "entry %d" % k)
    fold = ofl.Flow._chain_fold(objs, True)
    full = t - 1 if ref == 's' else 0
    fold_mask, chain_mask = fold[full].mask.cpu().numpy(), out[full].mask.cpu().numpy()
    assert (chain_mask <= fold_mask).all() and (chain_mask != fold_mask).any()
    assert fold[zero_at].vecs.data_ptr() == fold[co.walk_order(t, ref)[0]].vecs.data_ptr()      # the early exit: the operand itself


@pytest.mark.parametrize("ref", REFS)
def test_requires_grad_takes_the_fold_and_keeps_its_gradients(ref):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _native
    n, h, w, t = 2, 20, 28, 3
    flows, masks = co.case(n, h, w, ref, t)
    dev = _dev()

    def leaves():
        vs = [torch.from_numpy(np.array(f)).to(dev).requires_grad_() for f in flows]
        return vs, [ofl.Flow(v, ref, None if m is None else torch.from_numpy(np.array(m)).to(dev)) for v, m in zip(vs, masks)]

    weight = torch.from_numpy(np.random.RandomState(5).rand(n, 2, h, w).astype(np.float32)).to(dev)
    va, a = leaves()
    res = ofl.Flow.chain(a)
    assert res.vecs.grad_fn is not None and KERNEL not in _native.last_kernel_name()
    (res.vecs * weight).sum().backward()
    vb, b = leaves()
    fold = co.fold(b, ref)
    explicit = fold[-1] if ref == 's' else fold[0]
    (explicit.vecs * weight).sum().backward()
    _same_flows(res, explicit)
    for x, y in zip(va, vb):
        assert x.grad is not None and y.grad is not None and np.array_equal(_bits(x.grad), _bits(y.grad))
    assert any(bool(x.grad.any()) for x in va)
    # without gradients -- detached flows, or no_grad -- the new kernel runs
    vc, c = leaves()
    with torch.no_grad():
        quiet = ofl.Flow.chain(c)
    assert KERNEL in _native.last_kernel_name() and quiet.vecs.grad_fn is None
    _same_flows(quiet, explicit)
    _native.flow_flags(vc[0].detach())                        # (another kernel, so that the name below is this call's)
    assert KERNEL not in _native.last_kernel_name()
    plain = ofl.Flow.chain(_objs(flows, masks, ref))
    assert KERNEL in _native.last_kernel_name() and plain.vecs.grad_fn is None


def test_the_adapter_on_the_device():
    import oflibpytorch_amd as ofl
    n, h, w, t = 2, 8, 12, 3
    flows, masks = co.case(n, h, w, 't', t)
    vecs, valid, _ = co.reference(n, h, w, 't', t)
    dev = _dev()
    v, m = ofl.chain_flows([torch.from_numpy(np.array(f)).to(dev) for f in flows], 't',
                           masks=[None if k is None else torch.from_numpy(np.array(k)).to(dev) for k in masks])
    assert v.device.type == 'cuda' and np.array_equal(_bits(v), _bits(vecs[0])) and np.array_equal(_bits(m), _bits(valid[0]))


def test_c_abi_rejects_before_any_launch():
    from oflibpytorch_amd import _chain, _native
    lib = _chain._library()
    _native.flow_flags(torch.zeros(1, 2, 4, 4, device=_dev()))
    before = _native.last_kernel_name()
    assert KERNEL not in before
    for what, kw in co.rejected_calls():
        assert co.call_abi(lib, **kw) == -3, what              # OFL_E_ARG
        assert _native.last_kernel_name() == before, what      # nothing launched
    # ... and the same call with nothing wrong in it is taken
    dev = _dev()
    t, n, h, w = 3, 1, 4, 4
    fl = [torch.zeros(n, 2, h, w, device=dev) for _ in range(t)]
    out, om = torch.empty(n, 2, h, w, device=dev), torch.empty(n, h, w, dtype=torch.bool, device=dev)
    ptrs = (ctypes.c_void_p * t)(*[f.data_ptr() for f in fl])
    rc = co.call_abi(lib, t=t, n=n, h=h, w=w, flows=ptrs, bs=2 * h * w, masks=None, out=out.data_ptr(), out_mask=om.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and KERNEL in _native.last_kernel_name() and not bool(out.any()) and bool(om.all())
