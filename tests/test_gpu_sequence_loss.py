"""GPU tier of Flow.sequence_loss / sequence_stats against tests/sequence_loss_oracle.py.

Frames by H*W: 1, 5 and 4 pixels; the kernels' chunk of pixels per block (CHUNK) minus one, exact, plus one, and two chunks plus one; a
frame of a chunk and four pixels, whose second block holds one lane's group in the vector form; the odd sizes take the per-element form.
Every frame in a batch of 3, T in {1, 2, 12, 32}.  Bit for bit where the float64 sums are exact in any order (the oracle checks that of
every input itself), within the derived bounds on general inputs, and the properties: the batch, a second run, fp16 storage, slices of a
stacked tensor, no mask, a prediction without a gradient, an image without a valid pixel, the planted pixels."""
import functools
import math

import numpy as np
import pytest
import torch

import sequence_loss_oracle as so

pytestmark = pytest.mark.gpu

CHUNK = 2048                                         # OFL_SEQUENCE_LOSS_CHUNK: the pixels a block owns
FRAMES = [(1, 1), (1, 5), (2, 2), (1, CHUNK - 1), (32, CHUNK // 32), (1, CHUNK + 1), (1, 2 * CHUNK + 1), (4, CHUNK // 4 + 1)]
TS = [1, 2, 12, 32]
N = 3
UPSTREAM = np.array([0.75, -1.5, 2.0], np.float32)


def _dev():
    return torch.device('cuda', 0)


def _d(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x).copy()).to(_dev())
    return t.requires_grad_(True) if grad else t


def _kernel():
    from oflibpytorch_amd import _native
    return _native.last_kernel_name(demangle=False)


def _form(h, w):
    """The instantiation the launchers pick for contiguous fp32 tensors: the vector form where H*W is a multiple of 4"""
    return "ILb1E" if (h * w) % 4 == 0 else "ILb0E"


@functools.lru_cache(maxsize=None)
def _exact_case(h, w, t, penalty):
    cells = 4.0 if t == 32 else 64.0                 # (gamma = 0.5: the first of 32 weights is 2^-31)
    make = so.vectors_exact if penalty == 'l1' else so.vectors_pythagorean
    preds, gt = make(t, N, h, w, cells=cells)
    mask = so.masks(N, h, w)
    if h * w >= 8:
        so.plant(preds, gt, mask)
    so.require_exact(preds, gt, mask, 400.0, penalty, 0.5)
    return preds, gt, mask, so.compute(preds, gt, mask, 400.0, penalty)


@functools.lru_cache(maxsize=None)
def _general_case(h, w, t, penalty):
    preds, gt = so.vectors_general(t, N, h, w)
    mask = so.masks(N, h, w)
    return preds, gt, mask, so.compute(preds, gt, mask, 6.0, penalty)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("penalty", ['l1', 'l2'])
@pytest.mark.parametrize("t", TS)
@pytest.mark.parametrize("h,w", FRAMES)
def test_exact_inputs_bit_for_bit(h, w, t, penalty):
    """Inputs whose float64 sums are exact in any order: the whole record, the loss under gamma = 0.5 and both normalisations, and the
    'l1' gradients carry the oracle's bits; the 'l2' gradients are within 4 ulp32 (three float32 roundings, margin 2 x)"""
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _sequence_loss
    preds, gt, mask, ref = _exact_case(h, w, t, penalty)
    dp, dg, dm = [_d(p) for p in preds], _d(gt), _d(mask)
    rec = _sequence_loss.flow_sequence_loss(dp, dg, dm, 400.0, penalty, 'all')
    assert 'flow_sequence_loss_finish_kernel' in _kernel()
    assert rec.dtype == torch.float64 and rec.shape == (N, 2 * t + 4)
    assert np.array_equal(_bits(rec.cpu().numpy()), _bits(ref['record']))
    if h * w >= 8:                                   # the planted pixels: a magnitude of exactly max_flow, errors of exactly 1, 3, 5
        flat = ref['valid'].reshape(N, -1)
        assert not flat[:, 1].any() and np.array_equal(ref['e'][-1].reshape(N, -1)[:, 2:5], np.tile(np.float32([1, 3, 5]), (N, 1)))
    for normalise in ('all', 'valid'):
        want = so.loss64(ref['record'], h * w, 0.5, penalty, normalise).astype(np.float32)
        tp = [_d(p, grad=(i != 0 or t == 1)) for i, p in enumerate(preds)]           # prediction 0 of several wants no gradient
        loss = ofl.flow_sequence_loss(tp, dg, dm, gamma=0.5, penalty=penalty, normalise=normalise)
        assert loss.dtype == torch.float32 and np.array_equal(_bits(loss.detach().cpu().numpy()), _bits(want))
        loss.backward(_d(UPSTREAM))
        assert 'flow_sequence_loss_grad_kernel' + _form(h, w) in _kernel()
        grads = so.grads(preds, gt, mask, 400.0, penalty, normalise, 0.5, UPSTREAM)
        for i in range(t):
            if t > 1 and i == 0:
                assert tp[i].grad is None
                continue
            got = tp[i].grad.cpu().numpy()
            assert got.dtype == np.float32 and got.shape == (N, 2, h, w)
            if penalty == 'l1':
                assert np.array_equal(_bits(got), _bits(grads[i])), i
            else:
                assert np.all(np.abs(got.astype(np.float64) - grads[i]) <= 4 * so.ulp32(grads[i])), i
                assert not got[~np.broadcast_to(ref['valid'][:, None], got.shape)].any()


@pytest.mark.parametrize("penalty", ['l1', 'l2'])
@pytest.mark.parametrize("t", TS)
@pytest.mark.parametrize("h,w", FRAMES)
def test_general_inputs_within_the_derived_bounds(h, w, t, penalty):
    """N(0, 3) vectors, gamma = 0.8, max_flow = 6: the counts are exact, every sum is within count * 2^-52 relative of math.fsum of the
    oracle's float32 terms (the terms are >= 0), the loss within one ulp32 of the oracle's float64 value ((T + 2) * 2^-53
    relative from the float64 combination, and one rounding that may fall either side)"""
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _sequence_loss
    preds, gt, mask, ref = _general_case(h, w, t, penalty)
    dp, dg, dm = [_d(p) for p in preds], _d(gt), _d(mask)
    rec = _sequence_loss.flow_sequence_loss(dp, dg, dm, 6.0, penalty, 'all').cpu().numpy()
    assert 'flow_sequence_loss_finish_kernel' in _kernel()
    want = ref['record']
    counts = [0] + list(range(1 + 2 * t, 4 + 2 * t))
    assert np.array_equal(rec[:, counts], want[:, counts])
    sums = list(range(1, 1 + 2 * t))
    assert np.all(np.abs(rec[:, sums] - want[:, sums]) <= want[:, :1] * 2.0 ** -52 * want[:, sums])
    for normalise in ('all', 'valid'):
        loss = ofl.flow_sequence_loss(dp, dg, dm, max_flow=6.0, penalty=penalty, normalise=normalise).cpu().numpy()
        want64 = so.loss64(want, h * w, 0.8, penalty, normalise)
        ok = np.abs(loss.astype(np.float64) - want64) <= so.ulp32(want64)
        assert np.all(ok | (np.isnan(loss) & np.isnan(want64)))
    tp = [_d(p, grad=True) for p in preds]
    ofl.flow_sequence_loss(tp, dg, dm, max_flow=6.0, penalty=penalty, normalise='valid').backward(_d(UPSTREAM))
    assert 'flow_sequence_loss_grad_kernel' + _form(h, w) in _kernel()
    grads = so.grads(preds, gt, mask, 6.0, penalty, 'valid', 0.8, UPSTREAM)
    # the scale is formed from the kernel's sums' count only: the oracle's bits ('l1'), 4 ulp32 ('l2')
    for i in range(t):
        got = tp[i].grad.cpu().numpy()
        if penalty == 'l1':
            assert np.array_equal(_bits(got), _bits(grads[i])), i
        else:
            assert np.all(np.abs(got.astype(np.float64) - grads[i]) <= 4 * so.ulp32(grads[i])), i


def _run_raw(preds, gt, mask, penalty, normalise='valid', wants=None, gamma=0.8, max_flow=6.0, upstream=UPSTREAM):
    """(record, gradients) through the binding: tensors on the device in, tensors out"""
    from oflibpytorch_amd import _sequence_loss
    rec = _sequence_loss.flow_sequence_loss(preds, gt, mask, max_flow, penalty, normalise)
    assert 'flow_sequence_loss_finish_kernel' in _kernel()
    hw = int(gt.shape[-2]) * int(gt.shape[-1])
    scale = _sequence_loss.scale_of(_d(upstream), rec, hw, gamma, penalty, normalise)
    wants = [True] * len(preds) if wants is None else wants
    grads = _sequence_loss.flow_sequence_loss_grad(preds, gt, mask, max_flow, penalty, normalise, scale, wants)
    assert 'flow_sequence_loss_grad_kernel' in _kernel()
    return rec, grads


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


PROPERTY_FRAMES = [(1, 2 * CHUNK + 1), (4, CHUNK // 4 + 1)]


@pytest.mark.parametrize("penalty", ['l1', 'l2'])
@pytest.mark.parametrize("h,w", PROPERTY_FRAMES)
def test_an_image_carries_the_same_bits_alone_in_any_batch_and_on_a_second_run(h, w, penalty):
    t = 3
    preds, gt, mask, _ = _general_case(h, w, t, penalty)
    dp, dg, dm = [_d(p) for p in preds], _d(gt), _d(mask)
    rec, grads = _run_raw(dp, dg, dm, penalty)
    rec2, grads2 = _run_raw(dp, dg, dm, penalty)
    assert _same(rec, rec2) and all(_same(a, b) for a, b in zip(grads, grads2))
    order = [2, 0, 1]
    rec3, grads3 = _run_raw([p[order].contiguous() for p in dp], dg[order].contiguous(), dm[order].contiguous(), penalty,
                            upstream=UPSTREAM[order])
    assert _same(rec3, rec[order]) and all(_same(a, b[order]) for a, b in zip(grads3, grads))
    for k in range(N):
        one_rec, one_grads = _run_raw([p[k:k + 1] for p in dp], dg[k:k + 1], dm[k:k + 1], penalty, upstream=UPSTREAM[k:k + 1])
        assert _same(one_rec, rec[k:k + 1]) and all(_same(a, b[k:k + 1]) for a, b in zip(one_grads, grads))


@pytest.mark.parametrize("penalty", ['l1', 'l2'])
@pytest.mark.parametrize("h,w", PROPERTY_FRAMES)
def test_fp16_storage_gives_the_bits_of_its_exact_up_conversion(h, w, penalty):
    t = 3
    preds, gt, mask, _ = _general_case(h, w, t, penalty)
    hp, hg, dm = [_d(p.astype(np.float16)) for p in preds], _d(gt.astype(np.float16)), _d(mask)
    rec, grads = _run_raw(hp, hg, dm, penalty)
    rec32, grads32 = _run_raw([p.float() for p in hp], hg.float(), dm, penalty)
    assert _same(rec, rec32) and all(_same(a, b) for a, b in zip(grads, grads32))
    mixed = [hp[0], hp[1].float(), hp[2]]            # the storage kind is per prediction
    rec_m, grads_m = _run_raw(mixed, hg.float(), dm, penalty)
    assert _same(rec_m, rec32) and all(_same(a, b) for a, b in zip(grads_m, grads32))
    ref = so.compute([p.astype(np.float16) for p in preds], gt.astype(np.float16), mask, 6.0, penalty)['record']
    assert np.array_equal(rec.cpu().numpy()[:, 0], ref[:, 0])


@pytest.mark.parametrize("h,w", PROPERTY_FRAMES)
def test_slices_of_a_stacked_tensor_no_mask_and_a_prediction_without_a_gradient(h, w):
    import oflibpytorch_amd as ofl
    t, penalty = 3, 'l1'
    preds, gt, mask, _ = _general_case(h, w, t, penalty)
    dp, dg, dm = [_d(p) for p in preds], _d(gt), _d(mask)
    stack = _d(np.stack(preds))
    rec, grads = _run_raw(dp, dg, dm, penalty)
    rec_s, grads_s = _run_raw(list(stack.unbind(0)), dg, dm, penalty)
    assert _same(rec, rec_s) and all(_same(a, b) for a, b in zip(grads, grads_s))
    stack.requires_grad_(True)
    ofl.flow_sequence_loss(stack, dg, dm, max_flow=6.0, normalise='valid').backward(_d(UPSTREAM))
    assert stack.grad.shape == stack.shape and all(_same(stack.grad[i], grads[i]) for i in range(t))
    # only prediction 1 wants a gradient: the others are neither allocated nor written
    _, only = _run_raw(dp, dg, dm, penalty, wants=[False, True, False])
    assert only[0] is None and only[2] is None and _same(only[1], grads[1])
    # no mask: every pixel under max_flow; through the Flow API with consider_mask False, the predictions' masks not read
    want = so.compute(preds, gt, None, 6.0, penalty)['record']
    flows = [ofl.Flow(p, 't', ~dm) for p in dp]
    stats = ofl.Flow.sequence_stats(flows, ofl.Flow(dg, 't', dm), max_flow=6.0, consider_mask=False)
    assert np.array_equal(stats['count'].cpu().numpy(), want[:, 0]) and stats['count'].dtype == torch.int64
    assert np.array_equal(stats['within'].cpu().numpy(), want[:, 1 + 2 * t:] / want[:, :1])
    masked = ofl.Flow.sequence_stats(flows, ofl.Flow(dg, 't', dm), max_flow=6.0)
    assert np.array_equal(masked['count'].cpu().numpy(), so.compute(preds, gt, mask, 6.0, penalty)['record'][:, 0])
    loss = ofl.Flow.sequence_loss(flows, ofl.Flow(dg, 't', dm), max_flow=6.0)
    assert _same(loss, masked['loss']) and masked['epe'].shape == (N, t) and masked['terms'].shape == (N, t)
    assert np.allclose((masked['terms'] * masked['weights']).sum(1).cpu().numpy(), loss.cpu().numpy().astype(np.float64), rtol=1e-6)


@pytest.mark.parametrize("penalty", ['l1', 'l2'])
def test_an_image_without_a_valid_pixel(penalty):
    """NaN and a gradient of 0 under 'valid', exactly 0 under 'all'; the other images keep their bits"""
    import oflibpytorch_amd as ofl
    h, w, t = 4, CHUNK // 4 + 1, 3
    preds, gt, mask, _ = _general_case(h, w, t, penalty)
    empty = mask.copy()
    empty[1] = False
    gt2 = gt.copy()
    gt2[2] = 1000.0                                  # every magnitude of image 2 is over max_flow
    for normalise in ('all', 'valid'):
        tp = [_d(p, grad=True) for p in preds]
        loss = ofl.flow_sequence_loss(tp, _d(gt2), _d(empty), max_flow=6.0, penalty=penalty, normalise=normalise)
        loss.backward(_d(UPSTREAM))
        got = loss.detach().cpu().numpy()
        ref = so.loss64(so.compute(preds, gt2, empty, 6.0, penalty)['record'], h * w, 0.8, penalty, normalise)
        assert abs(got[0] - ref[0]) <= so.ulp32(ref[0]) and got[0] > 0
        if normalise == 'valid':
            assert np.isnan(got[1:]).all()
        else:
            assert np.array_equal(_bits(got[1:]), _bits(np.zeros(2, np.float32)))
        for p in tp:
            g = p.grad.cpu().numpy()
            assert np.array_equal(_bits(g[1:]), _bits(np.zeros_like(g[1:]))) and g[0].any()


def test_the_limits_of_the_binding():
    from oflibpytorch_amd import _sequence_loss
    dg = _d(np.zeros((1, 2, 2, 2), np.float32))
    with pytest.raises(RuntimeError, match="status -2"):
        _sequence_loss.flow_sequence_loss([dg] * 33, dg, None, 400.0, 'l1', 'all')
    with pytest.raises(RuntimeError, match="status -3"):
        _sequence_loss.flow_sequence_loss([dg], dg, None, math.nan, 'l1', 'all')
    rec = _sequence_loss.flow_sequence_loss([dg] * 32, dg, None, math.inf, 'l1', 'all')
    assert rec.shape == (1, 68) and rec[0, 0] == 4 and not rec[0, 1:65].any() and rec[0, 65:].tolist() == [4.0, 4.0, 4.0]
