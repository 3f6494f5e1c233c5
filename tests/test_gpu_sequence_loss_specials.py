"""Non-finite and extreme values through the sequence loss (the record rule of 3.16).

NaN, +-inf and +-FLT_MAX in one prediction at a valid pixel reach that prediction's two sums, its gradient at that pixel and the loss of
that image -- and `within` if it is the last prediction -- and nothing else: every other element keeps the bits of the run without the
special.  The same values at a pixel that is not valid change nothing, and in the ground truth they make the pixel not valid."""
import functools

import numpy as np
import pytest
import torch

import sequence_loss_oracle as so

pytestmark = pytest.mark.gpu

CHUNK = 2048
FRAMES = [(1, CHUNK + 1), (4, CHUNK // 4 + 1)]                           # the per-element and the vector form, two blocks each
SPECIALS = [np.nan, np.inf, -np.inf, so.FLT_MAX, -so.FLT_MAX]
N, T, IMG = 2, 3, 1
UPSTREAM = np.array([0.75, -1.5], np.float32)


def _d(x):
    return torch.from_numpy(np.ascontiguousarray(x).copy()).to(torch.device('cuda', 0))


@functools.lru_cache(maxsize=None)
def _case(h, w):
    preds, gt = so.vectors_general(T, N, h, w)
    mask = so.masks(N, h, w)
    valid = so.valid_of(gt, mask, 6.0)[IMG].reshape(-1)
    on, off = int(np.flatnonzero(valid)[-1]), int(np.flatnonzero(~valid)[-1])          # (in the second block both)
    assert on >= CHUNK or off >= CHUNK
    return preds, gt, mask, on, off


def _run(preds, gt, mask, penalty):
    """(records, loss, the T gradients) as numpy arrays: 'valid' normalisation, max_flow 6"""
    from oflibpytorch_amd import _native, _sequence_loss
    dp, dg, dm = [_d(p) for p in preds], _d(gt), _d(mask)
    rec = _sequence_loss.flow_sequence_loss(dp, dg, dm, 6.0, penalty, 'valid')
    assert 'flow_sequence_loss_finish_kernel' in _native.last_kernel_name(demangle=False)
    hw = gt.shape[2] * gt.shape[3]
    loss = _sequence_loss.loss_of(rec, hw, 0.8, penalty, 'valid')
    scale = _sequence_loss.scale_of(_d(UPSTREAM), rec, hw, 0.8, penalty, 'valid')
    grads = _sequence_loss.flow_sequence_loss_grad(dp, dg, dm, 6.0, penalty, 'valid', scale, [True] * T)
    assert 'flow_sequence_loss_grad_kernel' in _native.last_kernel_name(demangle=False)
    return rec.cpu().numpy(), loss.cpu().numpy(), [g.cpu().numpy() for g in grads]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _poke(a, img, comp, pixel, value):
    a = a.copy()
    a.reshape(a.shape[0], 2, -1)[img, comp, pixel] = value
    return a


@pytest.mark.parametrize("special", SPECIALS)
@pytest.mark.parametrize("which", [1, T - 1])
@pytest.mark.parametrize("penalty", ['l1', 'l2'])
@pytest.mark.parametrize("h,w", FRAMES)
def test_a_special_in_a_prediction(h, w, penalty, which, special):
    preds, gt, mask, on, off = _case(h, w)
    rec0, loss0, grads0 = _run(preds, gt, mask, penalty)
    # at a valid pixel
    poked = [(_poke(p, IMG, 0, on, special) if i == which else p) for i, p in enumerate(preds)]
    rec, loss, grads = _run(poked, gt, mask, penalty)
    may = np.zeros(rec.shape, bool)
    may[IMG, [1 + which, 1 + T + which]] = True
    if which == T - 1:
        may[IMG, 1 + 2 * T:] = True
    assert np.array_equal(_bits(rec[~may]), _bits(rec0[~may]))
    assert (_bits(rec[IMG, [1 + which, 1 + T + which]]) != _bits(rec0[IMG, [1 + which, 1 + T + which]])).all()
    want = so.compute(poked, gt, mask, 6.0, penalty)['record']
    both_nan = np.isnan(rec) & np.isnan(want)
    assert np.all(both_nan | (rec == want) | (np.abs(rec - want) <= want[:, :1] * 2.0 ** -52 * np.abs(want)))
    assert np.array_equal(rec[:, 1 + 2 * T:], want[:, 1 + 2 * T:])
    assert _bits(loss)[IMG] != _bits(loss0)[IMG] and _bits(loss)[1 - IMG] == _bits(loss0)[1 - IMG]
    exp = so.grads(poked, gt, mask, 6.0, penalty, 'valid', 0.8, UPSTREAM)
    for i in range(T):
        here = np.zeros(grads[i].shape, bool)
        if i == which:
            here.reshape(N, 2, -1)[IMG, :, on] = True
        # the scale of the image's other predictions is formed from the count alone: it keeps its bits
        assert np.array_equal(_bits(grads[i][~here]), _bits(grads0[i][~here])), i
        got, e = grads[i][here].astype(np.float64), exp[i][here].astype(np.float64)
        assert np.all((np.isnan(got) & np.isnan(e)) | (np.abs(got - e) <= (0 if penalty == 'l1' else 4) * so.ulp32(e))), i
    # at a pixel that is not valid: nothing changes
    poked = [(_poke(p, IMG, 1, off, special) if i == which else p) for i, p in enumerate(preds)]
    rec, loss, grads = _run(poked, gt, mask, penalty)
    assert np.array_equal(_bits(rec), _bits(rec0)) and np.array_equal(_bits(loss), _bits(loss0))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(grads, grads0))


@pytest.mark.parametrize("special", SPECIALS)
@pytest.mark.parametrize("penalty", ['l1', 'l2'])
@pytest.mark.parametrize("h,w", FRAMES)
def test_a_special_in_the_ground_truth_makes_the_pixel_not_valid(h, w, penalty, special):
    preds, gt, mask, on, _ = _case(h, w)
    rec0, _, grads0 = _run(preds, gt, mask, penalty)
    poked = _poke(gt, IMG, 1, on, special)
    rec, loss, grads = _run(preds, poked, mask, penalty)
    want = so.compute(preds, poked, mask, 6.0, penalty)['record']
    assert rec[IMG, 0] == rec0[IMG, 0] - 1 and np.array_equal(rec[:, 0], want[:, 0]) and np.isfinite(rec).all() and np.isfinite(loss).all()
    assert np.array_equal(rec[:, 1 + 2 * T:], want[:, 1 + 2 * T:])
    assert np.all(np.abs(rec - want) <= want[:, :1] * 2.0 ** -52 * want)
    assert np.array_equal(_bits(rec[1 - IMG]), _bits(rec0[1 - IMG]))
    for g, g0 in zip(grads, grads0):
        at = g.reshape(N, 2, -1)[IMG, :, on]
        assert np.array_equal(_bits(at), _bits(np.zeros(2, np.float32))) and g0.reshape(N, 2, -1)[IMG, :, on].any()
        assert np.array_equal(_bits(g[1 - IMG]), _bits(g0[1 - IMG]))
    # max_flow = inf lets every finite magnitude through, and still none that is not
    from oflibpytorch_amd import _sequence_loss
    count = _sequence_loss.flow_sequence_loss([_d(p) for p in preds], _d(poked), None, float('inf'), penalty, 'all')[:, 0].cpu().numpy()
    assert count.tolist() == [h * w, h * w - 1]
