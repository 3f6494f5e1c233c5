"""The flow propagation on dirty, guarded memory (tests/dirty_memory.py).

`_propagate` allocates its outputs, the result mask, the statistics of the backward (28 bytes a pixel), the scratch of the local backward
and the gradients with `torch.empty` under its own module-level name `torch`; here that name is a `dirty_memory.Harness` proxy, so every
such tensor is carved out of a buffer  guard | body | guard  whose body holds the fill byte.  For both forms, for the forward with and
without mask and statistics, for the whole backward and for each gradient alone: the same bits under the fills 0x00, 0xFF and 0x55
(nothing stale is read: every element of every output, every byte of the statistics and every element of the scratch that is read is
written first), no guard of any allocation is written, the inputs -- guarded copies, their guards holding the fill byte; the statistics
among them in the backward -- are unchanged, the result mask holds the bytes 0 and 1 only, and every allocation is made by a function
of the new module."""
import numpy as np
import pytest
import torch

import dirty_memory as dm
import propagate_oracle as po

pytestmark = pytest.mark.gpu

FRAMES = [(3, 5, 7), (2, 5, 35)]                     # Q = 35, narrower than a wave; Q = 175: three p-tiles, six q-chunks, two local tiles a row
C = 5
WHATS = ["forward", "forward-bare", "grads", "grad-query", "grad-key", "grad-flow"]


def _run(fill, n, h, w, radius, what):
    from oflibpytorch_amd import _propagate
    dev = torch.device('cuda', 0)
    query, key = (torch.from_numpy(x.copy()).to(dev) for x in po.features_general(n, C, h, w))
    flow = torch.from_numpy(po.vectors(n, h, w).copy()).to(dev)
    g = torch.from_numpy(po.upstream(n, h, w).copy()).to(dev)
    mask = torch.from_numpy(po.masks(n, h, w, radius)['one-image-masked'].copy()).to(dev)     # (a checkerboard, and empty pixels)
    stats = _propagate.flow_propagate(flow, mask, query, key, radius, True)[2]               # (made ahead: an input of the backward)
    harness = dm.Harness(fill)
    flow, mask, query, key, g, stats = harness.guard_all(flow, mask, query, key, g, stats)
    scratch = 0 if radius is None else 1                                                      # the local backward's workspace
    assert _propagate.torch is torch
    _propagate.torch = harness.proxy
    try:
        if what == "forward":
            res = list(_propagate.flow_propagate(flow, mask, query, key, radius, True))
            allocations, callers = 3, ["flow_propagate"]                                      # the vectors, the result mask, the statistics
        elif what == "forward-bare":
            res = [_propagate.flow_propagate(flow, None, query, key, radius, False)[0]]
            allocations, callers = 1, ["flow_propagate"]
        else:
            wants = {"grads": (True, True, True), "grad-query": (True, False, False), "grad-key": (False, True, False),
                     "grad-flow": (False, False, True)}[what]
            res = [d for d in _propagate.flow_propagate_grad(flow, mask, query, key, radius, stats, g, *wants) if d is not None]
            allocations, callers = sum(wants) + scratch, ["flow_propagate_grad"]
        torch.cuda.synchronize()
    finally:
        _propagate.torch = torch
    assert harness.callers() == callers
    assert len(harness.log) == allocations
    harness.check_guards()
    harness.check_inputs_unchanged()
    dm.assert_bool_bytes(res, what)
    return res


@pytest.mark.parametrize("what", WHATS)
@pytest.mark.parametrize("radius", [None, 1, 4])
@pytest.mark.parametrize("n,h,w", FRAMES)
def test_same_bits_under_every_fill(n, h, w, radius, what):
    results = [_run(fill, n, h, w, radius, what) for fill in dm.FILLS]
    for fill, res in zip(dm.FILLS[1:], results[1:]):
        dm.assert_same_bits(res, results[0], "%s under fill 0x%02X against 0x00" % (what, fill))
    query, key = po.features_general(n, C, h, w)                                              # ... and they are the right ones
    flow, g = po.vectors(n, h, w), po.upstream(n, h, w)
    mask = None if what == "forward-bare" else po.masks(n, h, w, radius)['one-image-masked']
    if what.startswith("forward"):
        r = po.compute(flow, mask, query, key, radius)
        want = [(r['out'], r['mag'], po.forward_shift(r['terms'])[:, None])]
        if what == "forward":
            assert np.array_equal(results[0][1].cpu().numpy(), r['valid']) and not r['valid'].all()
    else:
        r = po.grads(flow, mask, query, key, radius, g)
        every = [(r[k + '64'], r['mag_' + k], po.grad_shift(r['terms_' + k])) for k in ('d_query', 'd_key', 'd_flow')]
        want = {"grads": every, "grad-query": every[:1], "grad-key": every[1:2], "grad-flow": every[2:]}[what]
    for got, (exp, mag, shift) in zip(results[0], want):
        got = got.cpu().numpy()
        assert got.dtype == np.float32 and np.all(np.abs(got - exp) <= po.ulp32(exp) + 2.0 ** -np.asarray(shift, np.float64) * mag)
