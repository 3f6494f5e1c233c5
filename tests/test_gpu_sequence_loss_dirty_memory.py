"""The sequence loss on dirty, guarded memory (tests/dirty_memory.py).

`_sequence_loss` allocates the workspace and the records (`flow_sequence_loss`: two allocations) and one gradient per prediction that
wants one (`flow_sequence_loss_grad`) with `torch.empty` under its own module-level name `torch`; here that name is a
`dirty_memory.Harness` proxy, so every such tensor is carved out of a buffer  guard | body | guard  whose body holds the fill byte.  For
the forward, the statistics, the backward with all gradients and with one gradient alone: the same bits under the fills 0x00, 0xFF and
0x55 (nothing stale is read: every word of the workspace that the finish launch reads and every element of every output is written
first), no guard of any allocation is written, the inputs -- guarded copies, their guards holding the fill byte -- are unchanged, and
every allocation is made by the function the module's docstring names."""
import numpy as np
import pytest
import torch

import dirty_memory as dm
import sequence_loss_oracle as so

pytestmark = pytest.mark.gpu

CHUNK = 2048
FRAMES = [(3, 1, 5), (2, 1, 2 * CHUNK + 1), (2, 4, CHUNK // 4 + 1)]      # one block; three blocks, per-element; two blocks, vector form
T = 3
WHATS = ["forward", "stats", "grads", "grad-one"]
UPSTREAM = np.array([0.75, -1.5, 2.0], np.float32)


def _run(fill, n, h, w, penalty, what):
    from oflibpytorch_amd import _sequence_loss
    dev = torch.device('cuda', 0)
    preds, gt = so.vectors_general(T, n, h, w)
    tensors = [torch.from_numpy(p.copy()).to(dev) for p in preds] + [torch.from_numpy(gt.copy()).to(dev),
                                                                    torch.from_numpy(so.masks(n, h, w).copy()).to(dev)]
    rec = _sequence_loss.flow_sequence_loss(tensors[:T], tensors[T], tensors[T + 1], 6.0, penalty, 'valid')      # (made ahead)
    scale = _sequence_loss.scale_of(torch.from_numpy(UPSTREAM[:n].copy()).to(dev), rec, h * w, 0.8, penalty, 'valid')
    harness = dm.Harness(fill)
    guarded = harness.guard_all(*tensors, scale)
    dp, dg, dmask, scale = list(guarded[:T]), guarded[T], guarded[T + 1], guarded[T + 2]
    assert _sequence_loss.torch is torch
    _sequence_loss.torch = harness.proxy
    try:
        if what == "forward":
            res = [_sequence_loss.flow_sequence_loss(dp, dg, dmask, 6.0, penalty, 'valid')]
            allocations, callers = 2, ["flow_sequence_loss"]                                  # the workspace, the records
        elif what == "stats":
            stats = _sequence_loss.sequence_stats(dp, dg, dmask, 0.8, 6.0, penalty, 'valid')
            res = [stats[k] for k in sorted(stats)]
            allocations, callers = 2, ["flow_sequence_loss"]
        else:
            wants = [True] * T if what == "grads" else [False, True, False]
            res = [g for g in _sequence_loss.flow_sequence_loss_grad(dp, dg, dmask, 6.0, penalty, 'valid', scale, wants) if g is not None]
            allocations, callers = sum(wants), ["flow_sequence_loss_grad"]
        torch.cuda.synchronize()
    finally:
        _sequence_loss.torch = torch
    assert harness.callers() == callers
    assert len(harness.log) == allocations
    harness.check_guards()
    harness.check_inputs_unchanged()
    return res


@pytest.mark.parametrize("what", WHATS)
@pytest.mark.parametrize("penalty", ['l1', 'l2'])
@pytest.mark.parametrize("n,h,w", FRAMES)
def test_same_bits_under_every_fill(n, h, w, penalty, what):
    results = [_run(fill, n, h, w, penalty, what) for fill in dm.FILLS]
    for fill, res in zip(dm.FILLS[1:], results[1:]):
        dm.assert_same_bits(res, results[0], "%s under fill 0x%02X against 0x00" % (what, fill))
    preds, gt = so.vectors_general(T, n, h, w)                                                # ... and they are the right ones
    mask = so.masks(n, h, w)
    rec = so.compute(preds, gt, mask, 6.0, penalty)['record']
    if what == "forward":
        got = results[0][0].cpu().numpy()
        assert np.array_equal(got[:, 0], rec[:, 0]) and np.all(np.abs(got - rec) <= rec[:, :1] * 2.0 ** -52 * rec)
    elif what == "stats":
        count, _, loss = (results[0][k].cpu().numpy() for k in range(3))                      # count, epe, loss (sorted keys)
        want = so.loss64(rec, h * w, 0.8, penalty, 'valid')
        assert np.array_equal(count, rec[:, 0]) and np.all(np.abs(loss - want) <= so.ulp32(want))
    else:
        grads = so.grads(preds, gt, mask, 6.0, penalty, 'valid', 0.8, UPSTREAM[:n])
        for got, exp in zip(results[0], grads if what == "grads" else grads[1:2]):
            got = got.cpu().numpy()
            assert got.dtype == np.float32 and np.all(np.abs(got.astype(np.float64) - exp) <= (0 if penalty == 'l1' else 4) * so.ulp32(exp))
