"""Dirty, guarded memory for the primitives of `oflibpytorch_amd._native` (a helper module, not a test; test modules import it).

`_native` allocates every output, valid map, flag word and workspace with `torch.empty` / `torch.zeros`.  In a test process most of
that memory happens to be zero or to hold an earlier correct result, so a kernel that reads a word before the launch that clears it,
skips an output element on a tail, or stores a few elements past a row passes everything.  `Harness` makes both deterministic:

* for the duration of a `with` block the name `torch` seen by `_native` (and `_autograd`) is a proxy that forwards every attribute to
  the real module except `empty` and `zeros`.  `torch.empty` itself is never patched;
* the proxy's `empty` / `zeros` carve the tensor out of one flat uint8 buffer  GUARD | body | GUARD  on the requested device.  GUARD
  is 4096 bytes, a multiple of the allocator's 512-byte rounding, so the body is aligned exactly as a real allocation is.  The body
  of an `empty` is filled with the case's FILL BYTE, that of a `zeros` with 0; both guards hold a position-dependent canary that is
  never 0x00, 0xFF or the fill byte, so a run of stray zeros or NaNs cannot reproduce it;
* `check_guards()` compares every guard of every logged allocation with its canary, byte for byte;
* `guarded(t)` copies an INPUT into the body of such a buffer whose guards hold the fill byte (a read outside the input that
  influences anything then changes the result between fills); `check_inputs_unchanged()` compares the input's bytes -- and its
  guards -- with what they were.

Fill bytes, in this order: 0x00 (the control: what a fresh process mostly sees), 0xFF (float NaN, int32 -1, a bool byte that is
neither 0 nor 1), 0x55 (large finite floats, int32 1431655765).
"""
import sys

import torch

GUARD = 4096                       # bytes on either side of a body: a multiple of 512, so the body keeps the allocator's alignment
FILLS = (0x00, 0xFF, 0x55)
_PATCHED = ("oflibpytorch_amd._native", "oflibpytorch_amd._autograd")


def canary(nbytes: int, fill: int, phase: int = 0) -> torch.Tensor:
    """uint8[nbytes] on the CPU: (i * 37 + 11) & 0xFF at position i + phase, with 0x00, 0xFF and the fill byte remapped."""
    i = torch.arange(phase, phase + nbytes, dtype=torch.int64)
    v = (i * 37 + 11) & 0xFF
    for bad, to in ((0x00, 0x5A), (0xFF, 0xA6), (fill, 0xC3)):
        v = torch.where(v == bad, torch.full_like(v, to), v)
    for bad in (0x00, 0xFF, fill):
        assert not bool((v == bad).any())
    return v.to(torch.uint8)


class _Alloc(object):
    __slots__ = ("caller", "shape", "dtype", "fill", "buffer", "nbytes", "kind", "zeros")

    def __init__(self, caller, shape, dtype, fill, buffer, nbytes, kind, zeros):
        self.caller, self.shape, self.dtype, self.fill = caller, shape, dtype, fill
        self.buffer, self.nbytes, self.kind, self.zeros = buffer, nbytes, kind, zeros

    def __iter__(self):            # (caller function name in _native, shape, dtype, fill, buffer)
        return iter((self.caller, self.shape, self.dtype, self.fill, self.buffer))

    def describe(self):
        return "%s %s%s %s in %s()" % ("zeros" if self.zeros else "empty", self.kind, tuple(self.shape), self.dtype, self.caller)


class _TorchProxy(object):
    """`torch` as `_native` sees it inside a Harness: everything but `empty` and `zeros` is the real module's."""

    def __init__(self, harness):
        object.__setattr__(self, "_harness", harness)

    def __getattr__(self, name):
        return getattr(torch, name)

    def __setattr__(self, name, value):
        raise AttributeError("the proxy is read-only")

    def empty(self, *size, **kw):
        return self._harness._allocate(size, kw, zeros=False)

    def zeros(self, *size, **kw):
        return self._harness._allocate(size, kw, zeros=True)


def _shape_of(size):
    if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
        size = tuple(size[0])
    return tuple(int(s) for s in size)


class Harness(object):
    """One run of one case under one fill byte.  Use as a context manager around the calls into the package."""

    def __init__(self, fill: int):
        assert 0 <= fill <= 0xFF
        self.fill = int(fill)
        self.log = []              # _Alloc per proxy allocation, in order
        self.inputs = []           # (name, buffer, nbytes, saved copy of the whole buffer)
        self._saved = None
        self._canaries = {}
        self.proxy = _TorchProxy(self)    # what `_native` sees as `torch` inside the `with` block

    # -- the proxy's life -------------------------------------------------------------------------------------------------------
    def __enter__(self):
        import oflibpytorch_amd._autograd  # noqa: F401  (so that it is patched too if it ever allocates)
        import oflibpytorch_amd._native  # noqa: F401
        assert self._saved is None
        self._saved = {}
        for name in _PATCHED:
            mod = sys.modules[name]
            self._saved[name] = mod.torch
            assert self._saved[name] is torch, "%s.torch is already replaced" % name
            mod.torch = self.proxy
        return self

    def __exit__(self, *exc):
        for name, real in self._saved.items():
            sys.modules[name].torch = real
        self._saved = None
        return False

    # -- allocation ---------------------------------------------------------------------------------------------------------------
    def _canary(self, device, side):
        key = (str(device), side)
        if key not in self._canaries:
            self._canaries[key] = canary(GUARD, self.fill, 0 if side == 0 else GUARD // 2 + 1).to(device)
        return self._canaries[key]

    def _carve(self, shape, dtype, device, memory_format, body_fill, guard_fill):
        """(tensor over the body, flat buffer, body bytes).  guard_fill None: the canary."""
        meta = torch.empty(shape, dtype=dtype, device='meta', memory_format=memory_format)
        strides = meta.stride()
        numel = meta.numel()
        esize = meta.element_size()
        span = 0 if numel == 0 else 1 + sum((s - 1) * st for s, st in zip(shape, strides))
        assert span == numel, "only dense memory formats"
        nbytes = numel * esize
        assert GUARD % 512 == 0 and GUARD % esize == 0
        buf = torch.empty(GUARD + nbytes + GUARD, dtype=torch.uint8, device=device)
        if guard_fill is None:
            buf[:GUARD].copy_(self._canary(buf.device, 0))
            buf[GUARD + nbytes:].copy_(self._canary(buf.device, 1))
        else:
            buf[:GUARD].fill_(guard_fill)
            buf[GUARD + nbytes:].fill_(guard_fill)
        buf[GUARD:GUARD + nbytes].fill_(body_fill)
        out = buf.view(dtype).as_strided(shape, strides, GUARD // esize)      # (both guards and the body are multiples of esize)
        assert numel == 0 or out.data_ptr() == buf.data_ptr() + GUARD
        return out, buf, nbytes

    def _allocate(self, size, kw, zeros):
        kw = dict(kw)
        dtype = kw.pop("dtype", None) or torch.get_default_dtype()
        device = torch.device(kw.pop("device", None) or "cpu")
        memory_format = kw.pop("memory_format", torch.contiguous_format)
        assert not kw, "the proxy's empty / zeros take shape, dtype, device, memory_format: %s" % sorted(kw)
        shape = _shape_of(size)
        caller = sys._getframe(2).f_code.co_name
        out, buf, nbytes = self._carve(shape, dtype, device, memory_format, 0 if zeros else self.fill, None)
        self.log.append(_Alloc(caller, shape, dtype, self.fill, buf, nbytes, "", zeros))
        return out

    # -- inputs ---------------------------------------------------------------------------------------------------------------------
    def guarded(self, t, name="input"):
        """`t` copied into the body of a buffer whose guards hold the fill byte; None and broadcast (`expand`ed) inputs pass through."""
        if t is None or not isinstance(t, torch.Tensor):
            return t
        if t.numel() == 0 or any(st == 0 and s > 1 for s, st in zip(t.shape, t.stride())):
            return t
        fmt = torch.contiguous_format
        if t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last):
            fmt = torch.channels_last
        out, buf, nbytes = self._carve(tuple(t.shape), t.dtype, t.device, fmt, 0, self.fill)
        out.copy_(t.detach())
        if t.requires_grad:
            out.requires_grad_(True)
        self.inputs.append((name, buf, nbytes, buf.clone()))
        return out

    def guard_all(self, *tensors):
        return tuple(self.guarded(t, "input %d" % i) for i, t in enumerate(tensors))

    # -- checks ---------------------------------------------------------------------------------------------------------------------
    def callers(self):
        return sorted(set(a.caller for a in self.log))

    def check_guards(self):
        """Every guard of every logged allocation equals its canary."""
        for k, a in enumerate(self.log):
            for side, lo in ((0, 0), (1, GUARD + a.nbytes)):
                got = a.buffer[lo:lo + GUARD]
                bad = (got != self._canary(a.buffer.device, side)).nonzero()
                if bad.numel():
                    first, last = int(bad[0]), int(bad[-1])
                    where = "before" if side == 0 else "after"
                    off = (first - GUARD, last - GUARD) if side == 0 else (first, last)
                    raise AssertionError(
                        "fill 0x%02X: allocation %d (%s) was written %s its body: %d bytes differ, first at offset %d, last at %d "
                        "(relative to the %s of the body)" % (self.fill, k, a.describe(), where, int(bad.numel()), off[0], off[1],
                                                               "start" if side == 0 else "end"))

    def check_inputs_unchanged(self):
        for name, buf, nbytes, saved in self.inputs:
            bad = (buf != saved).nonzero()
            if bad.numel():
                first, last = int(bad[0]) - GUARD, int(bad[-1]) - GUARD
                raise AssertionError("fill 0x%02X: %s (%d bytes) or its guards were written: %d bytes differ, first at offset %d, "
                                     "last at %d of the input" % (self.fill, name, nbytes, int(bad.numel()), first, last))


# -- comparisons ------------------------------------------------------------------------------------------------------------------------
def as_bytes(t: torch.Tensor) -> torch.Tensor:
    """The tensor's elements as uint8, in logical order (NaN payloads and bool bytes count)."""
    t = t.detach()
    if t.dtype == torch.bool:
        return t.contiguous().view(torch.uint8).reshape(-1)
    return t.contiguous().reshape(-1).view(torch.uint8)


def flatten(res):
    """The tensors of a (nested) result, in order, with None kept as a placeholder."""
    if res is None or isinstance(res, torch.Tensor):
        return [res]
    if isinstance(res, (tuple, list)):
        out = []
        for r in res:
            out.extend(flatten(r))
        return out
    return []


def assert_same_bits(got, ref, what):
    a, b = flatten(got), flatten(ref)
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), "%s: result %d" % (what, k)
        if x is None:
            continue
        assert x.dtype == y.dtype and x.shape == y.shape and x.stride() == y.stride(), "%s: result %d: %s %s vs %s %s" % (
            what, k, x.dtype, tuple(x.shape), y.dtype, tuple(y.shape))
        xb, yb = as_bytes(x), as_bytes(y)
        if not torch.equal(xb, yb):
            bad = (xb != yb).nonzero().reshape(-1)
            e = x.element_size()
            raise AssertionError("%s: result %d (%s %s) differs in %d bytes, elements %d ... %d" % (
                what, k, x.dtype, tuple(x.shape), int(bad.numel()), int(bad[0]) // e, int(bad[-1]) // e))


def assert_bool_bytes(res, what):
    """Every bool output holds only the bytes 0 and 1."""
    for k, x in enumerate(flatten(res)):
        if x is not None and x.dtype == torch.bool:
            b = as_bytes(x)
            assert int(b.max()) <= 1 if b.numel() else True, "%s: bool result %d holds a byte that is neither 0 nor 1" % (what, k)
