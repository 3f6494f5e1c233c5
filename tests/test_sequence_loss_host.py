"""CPU tier of Flow.sequence_loss: the oracle (tests/sequence_loss_oracle.py) against RAFT's loop written in torch float64
and its autograd, four mutants that the comparison must tell apart, the exact inputs of the GPU tier, the host logic of the API with the
native calls served by the oracle, every argument check that needs no device, and the C ABI's declarations and argument checks.  No
device."""
import ctypes
import math

import numpy as np
import pytest
import torch

import sequence_loss_oracle as so

SHAPES = ((5, 7), (9, 11))
N = 2


@pytest.fixture
def sl_native(oracle_native, monkeypatch):
    from oflibpytorch_amd import _sequence_loss
    monkeypatch.setattr(_sequence_loss, "flow_sequence_loss", so.fake_flow_sequence_loss)
    monkeypatch.setattr(_sequence_loss, "flow_sequence_loss_grad", so.fake_flow_sequence_loss_grad)
    return _sequence_loss


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x).copy())


def raft_loop(preds, gt, valid, gamma, max_flow, penalty='l1', normalise='all'):
    """RAFT's sequence_loss (train.py) on torch tensors, per image: `valid` a float mask, the loop, the weights and the magnitude test as
    published; 'l2' takes the norm of the difference, 'valid' divides by the terms of the valid pixels.  Returns [N]; under
    ('l1', 'all') its mean is RAFT's scalar."""
    n_predictions = len(preds)
    mag = torch.sum(gt ** 2, dim=1).sqrt()
    valid = (valid >= 0.5) & (mag < max_flow)
    flow_loss = 0.0
    for i in range(n_predictions):
        i_weight = gamma ** (n_predictions - i - 1)
        if penalty == 'l1':
            i_loss = (preds[i] - gt).abs()
        else:
            i_loss = torch.sum((preds[i] - gt) ** 2, dim=1, keepdim=True).sqrt()
        masked = valid[:, None] * i_loss
        if normalise == 'all':
            flow_loss = flow_loss + i_weight * masked.mean(dim=(1, 2, 3))
        else:
            flow_loss = flow_loss + i_weight * masked.sum(dim=(1, 2, 3)) / (valid.sum(dim=(1, 2)) * i_loss.shape[1])
    return flow_loss


# ---- the oracle computes RAFT's expression -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_flow", [6.0, math.inf])
@pytest.mark.parametrize("normalise", ['all', 'valid'])
@pytest.mark.parametrize("penalty", ['l1', 'l2'])
@pytest.mark.parametrize("t", [1, 3, 12])
@pytest.mark.parametrize("h,w", SHAPES)
def test_float64_evaluation_is_rafts_loop_and_its_autograd(h, w, t, penalty, normalise, max_flow):
    """A batch of 2, a mask with holes: the oracle's float64 evaluation and its gradients against RAFT's loop in torch float64 and torch's
    autograd of it, within 1e-12 of each result's scale"""
    preds, gt = so.vectors_general(t, N, h, w)
    mask = so.masks(N, h, w)
    g = np.array([0.75, -1.5])
    rec = so.compute(preds, gt, mask, max_flow, penalty, wide=True)['record']
    assert 0 < rec[:, 0].min() and (math.isinf(max_flow) or rec[:, 0].max() < mask.reshape(N, -1).sum(1).max())     # the test cuts pixels
    got = so.loss64(rec, h * w, 0.8, penalty, normalise)
    grads = so.grads(preds, gt, mask, max_flow, penalty, normalise, 0.8, g, wide=True)
    tp = [_t(p).double().requires_grad_(True) for p in preds]
    want = raft_loop(tp, _t(gt).double(), _t(mask).double(), 0.8, max_flow, penalty, normalise)
    (want * _t(g)).sum().backward()
    scale = float(want.detach().abs().max())
    err = float(np.abs(got - want.detach().numpy()).max())
    print("%d x %d T %d %s %s: largest |oracle - RAFT| = %.3e of a scale %.3e" % (h, w, t, penalty, normalise, err, scale))
    assert scale > 0 and err <= 1e-12 * scale
    for i in range(t):
        gs = float(tp[i].grad.abs().max())
        assert gs > 0 and np.abs(grads[i] - tp[i].grad.numpy()).max() <= 1e-12 * gs, i
    if (penalty, normalise) == ('l1', 'all'):
        scalar = raft_loop([p.detach() for p in tp], _t(gt).double(), _t(mask).double(), 0.8, max_flow).mean()
        assert abs(got.mean() - float(scalar)) <= 1e-12 * scale
    # the definition's float32 terms are close to the float64 ones
    rec32 = so.compute(preds, gt, mask, max_flow, penalty)['record']
    assert np.array_equal(rec32[:, 0], rec[:, 0]) and np.abs(rec32 - rec).max() <= 1e-5 * np.abs(rec).max()


@pytest.mark.parametrize("mutant", so.MUTANTS)
def test_mutants_fail_the_comparison(mutant):
    """The weights reversed, the magnitude test on the prediction, <= for < at a planted pixel of magnitude exactly max_flow and the
    divisor without its factor 2 each compute another function: each must miss RAFT's loop by more than a tenth of the loss's scale, on
    inputs where the oracle itself is within 1e-12"""
    (h, w), t, max_flow = SHAPES[0], 3, 400.0
    preds, gt = so.vectors_general(t, N, h, w)
    preds = [(gt + (p - gt) * np.float32(4.0 ** (t - 1 - i))).astype(np.float32) for i, p in enumerate(preds)]     # steep convergence
    gt[:, :, :, ::2] = np.float32(1000.0)                      # every other column of the ground truth is faster than max_flow: not valid
    mask = so.masks(N, h, w)
    gt[:, 0, 1, 1], gt[:, 1, 1, 1] = 240.0, 320.0              # a magnitude of exactly 400 where the predictions are far off
    mask[:, 1, 1] = True
    for p in preds:
        p[:, :, 1, 1] = 0.0
    assert np.array_equal(so.valid_of(gt, mask, max_flow)[:, 1, 1], [False, False])
    want = raft_loop([_t(p).double() for p in preds], _t(gt).double(), _t(mask).double(), 0.8, max_flow).numpy()
    scale = np.abs(want).max()

    def miss(mutant):
        rec = so.compute(preds, gt, mask, max_flow, 'l1', wide=True, mutant=mutant)['record']
        return np.abs(so.loss64(rec, h * w, 0.8, 'l1', 'all', mutant=mutant) - want).max()
    print("%s: misses by %.3f of the scale" % (mutant, miss(mutant) / scale))
    assert miss(mutant) > 0.1 * scale
    assert miss(None) <= 1e-12 * scale


@pytest.mark.parametrize("t", [1, 2, 12, 32])
def test_the_exact_inputs_are_what_they_say(t):
    """The bit-for-bit tier of the GPU tests rests on these: the oracle's own check passes on them, fails on general inputs, and the
    planted pixels are what their names say"""
    n, h, w = 2, 5, 7
    mask = so.masks(n, h, w)
    preds, gt = so.vectors_exact(t, n, h, w)
    so.plant(preds, gt, mask)
    so.require_exact(preds, gt, mask, 400.0, 'l1', 0.5)
    r = so.compute(preds, gt, mask, 400.0, 'l1')
    flat = lambda a: a.reshape(n, -1)                                      # noqa: E731
    assert not flat(r['valid'])[:, 1].any() and flat(r['valid'])[:, 2:6].all()
    assert np.array_equal(flat(r['e'][-1])[:, 2:5], np.tile(np.float32([1, 3, 5]), (n, 1)))
    assert (flat(r['e'][-1])[:, 5] == 0).all()
    e_last, v = flat(r['e'][-1]), flat(r['valid'])
    for j, thr in enumerate(so.WITHIN):                                     # strictly below: the planted pixel is not within
        assert np.array_equal(r['record'][:, 1 + 2 * t + j], (v & (e_last < thr)).sum(1))
        assert (r['record'][:, 1 + 2 * t + j] < (v & (e_last <= thr)).sum(1)).all()
    preds, gt = so.vectors_pythagorean(t, n, h, w)
    so.plant(preds, gt, mask)
    so.require_exact(preds, gt, mask, 400.0, 'l2', 0.5)
    e = so.compute(preds, gt, mask, 400.0, 'l2')['e'].astype(np.float64)
    assert np.array_equal(e * 64.0, np.round(e * 64.0))
    with pytest.raises(AssertionError):
        so.require_exact(*so.vectors_general(t, n, h, w), mask, 400.0, 'l1')
    if t > 1:
        with pytest.raises(AssertionError):                                 # weights that are no powers of two
            so.require_exact(preds, gt, mask, 400.0, 'l2', 0.8)


def test_non_finite_values_follow_the_record_rule():
    n, h, w, t = 1, 3, 4, 3
    preds, gt = so.vectors_general(t, n, h, w)
    mask = np.ones((n, h, w), bool)
    mask[0, 2, 3] = False
    clean = so.compute(preds, gt, mask)['record']
    for special in (np.nan, np.inf, -np.inf, so.FLT_MAX, -so.FLT_MAX):
        p = [a.copy() for a in preds]
        p[1][0, 0, 1, 2] = special                                          # a valid pixel of prediction 1
        rec = so.compute(p, gt, mask)['record']
        changed = np.zeros(rec.shape, bool)
        changed[0, [1 + 1, 1 + t + 1]] = True
        assert (rec[changed] != clean[changed]).all() and np.array_equal(rec[~changed], clean[~changed])
        assert np.isnan(rec[changed]).all() if np.isnan(special) else np.isinf(rec[changed]).any()
        p = [a.copy() for a in preds]
        p[1][0, 0, 2, 3] = special                                          # a pixel that is not valid: nothing changes
        assert np.array_equal(so.compute(p, gt, mask)['record'], clean)
        g = gt.copy()
        g[0, 1, 0, 0] = special                                             # in the ground truth: the pixel is not valid
        r = so.compute(preds, g, mask)
        assert not r['valid'][0, 0, 0] and r['record'][0, 0] == clean[0, 0] - 1 and np.isfinite(r['record']).all()


# ---- the host logic of the API, the oracle in the bindings' place ---------------------------------------------------------------------
@pytest.mark.parametrize("penalty,normalise", [(None, None), ('l1', 'valid'), ('l2', 'all'), ('l2', 'valid')])
def test_values_shapes_stats_and_the_wrapper(sl_native, penalty, normalise):
    import oflibpytorch_amd as ofl
    (h, w), t = SHAPES[0], 3
    preds, gt = so.vectors_general(t, N, h, w)
    mask = so.masks(N, h, w)
    pen, norm = penalty or 'l1', normalise or 'all'
    flows = [ofl.Flow(_t(p), 't', _t(~mask)) for p in preds]               # the predictions' masks are not read
    truth = ofl.Flow(_t(gt), 't', _t(mask))
    rec = so.compute(preds, gt, mask, 6.0, pen)['record']
    want = so.loss64(rec, h * w, 0.8, pen, norm)
    loss = ofl.Flow.sequence_loss(flows, truth, max_flow=6.0, penalty=penalty, normalise=normalise)
    assert loss.dtype == torch.float32 and loss.shape == (N,) and not loss.requires_grad
    assert np.abs(loss.numpy() - want).max() <= so.ulp32(want).max()
    assert np.array_equal(ofl.Flow.sequence_loss(tuple(flows), truth, 0.8, 6.0, penalty, normalise).numpy(), loss.numpy())
    stats = ofl.Flow.sequence_stats(flows, truth, max_flow=6.0, penalty=penalty, normalise=normalise)
    assert sorted(stats) == ['count', 'epe', 'loss', 'terms', 'weights', 'within']
    assert stats['count'].dtype == torch.int64 and np.array_equal(stats['count'].numpy(), rec[:, 0])
    assert np.array_equal(stats['loss'].numpy(), loss.numpy())
    assert stats['weights'].dtype == torch.float64 and stats['weights'].tolist() == so.weights(t, 0.8)
    div = so.divisor(rec, h * w, pen, norm)
    assert stats['terms'].shape == (N, t) and np.array_equal(stats['terms'].numpy(), rec[:, 1:1 + t] / div[:, None])
    assert np.array_equal(stats['epe'].numpy(), rec[:, 1 + t:1 + 2 * t] / rec[:, :1])
    assert stats['within'].shape == (N, 3) and np.array_equal(stats['within'].numpy(), rec[:, 1 + 2 * t:] / rec[:, :1])
    # consider_mask False: every pixel under max_flow; the defaults are RAFT's
    rec_all = so.compute(preds, gt, None, 400.0, pen)['record']
    got = ofl.Flow.sequence_loss(flows, truth, penalty=penalty, normalise=normalise, consider_mask=False)
    assert np.abs(got.numpy() - so.loss64(rec_all, h * w, 0.8, pen, norm)).max() <= so.ulp32(want).max()
    # the wrapper: a list, a stacked tensor, 3-D input
    got = ofl.flow_sequence_loss([_t(p) for p in preds], _t(gt), _t(mask), max_flow=6.0, penalty=penalty, normalise=normalise)
    assert got.shape == (N,) and np.array_equal(got.numpy(), loss.numpy())
    got = ofl.flow_sequence_loss(_t(np.stack(preds)), _t(gt), _t(mask), max_flow=6.0, penalty=penalty, normalise=normalise)
    assert np.array_equal(got.numpy(), loss.numpy())
    got = ofl.flow_sequence_loss(_t(np.stack(preds)[:, 1]), _t(gt[1]), _t(mask[1]), max_flow=6.0, penalty=penalty, normalise=normalise)
    assert got.shape == () and got.numpy() == loss.numpy()[1]
    # an image without a valid pixel
    none = ofl.Flow.sequence_loss(flows, ofl.Flow(_t(gt), 't', _t(np.zeros_like(mask))), penalty=penalty, normalise=normalise)
    assert np.isnan(none.numpy()).all() if norm == 'valid' else np.array_equal(none.numpy(), np.zeros(N, np.float32))


@pytest.mark.parametrize("penalty,normalise", [('l1', 'all'), ('l2', 'valid')])
def test_requires_grad_routing(sl_native, monkeypatch, penalty, normalise):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _autograd
    (h, w), t = SHAPES[0], 3
    preds, gt = so.vectors_general(t, N, h, w)
    mask = so.masks(N, h, w)
    g = np.array([0.75, -1.5], np.float32)
    calls = []
    real = so.fake_flow_sequence_loss_grad

    def spy(preds, gt, gt_mask, max_flow, penalty, normalise, scale, wants):
        calls.append(list(wants))
        assert scale.dtype == torch.float32 and scale.shape == (gt.shape[0], t)
        return real(preds, gt, gt_mask, max_flow, penalty, normalise, scale, wants)
    monkeypatch.setattr(sl_native, "flow_sequence_loss_grad", spy)
    want = so.grads(preds, gt, mask, 6.0, penalty, normalise, 0.8, g)
    tp = [_t(p).requires_grad_(i != 1) for i, p in enumerate(preds)]       # prediction 1 wants no gradient
    tg, tm = _t(gt).requires_grad_(True), _t(mask)
    assert issubclass(_autograd.SequenceLossFn, torch.autograd.Function)
    loss = ofl.Flow.sequence_loss([ofl.Flow(p, 't') for p in tp], ofl.Flow(tg, 't', tm), max_flow=6.0, penalty=penalty, normalise=normalise)
    assert loss.requires_grad and type(loss.grad_fn).__name__ == "SequenceLossFnBackward"
    loss.backward(_t(g))
    assert calls == [[True, False, True]]
    assert tp[1].grad is None and tg.grad is None
    for i in (0, 2):
        assert tp[i].grad.dtype == torch.float32 and np.array_equal(tp[i].grad.numpy(), want[i])
    with torch.no_grad():
        assert not ofl.Flow.sequence_loss([ofl.Flow(p, 't') for p in tp], ofl.Flow(tg, 't', tm)).requires_grad
    # nothing requires a gradient: no grad_fn
    assert ofl.flow_sequence_loss([_t(p) for p in preds], _t(gt)).grad_fn is None
    # a stacked tensor gets a gradient of the stack's shape, its slices used in place
    stack = _t(np.stack(preds)).requires_grad_(True)
    ofl.flow_sequence_loss(stack, _t(gt), tm, max_flow=6.0, penalty=penalty, normalise=normalise).backward(_t(g))
    assert stack.grad.shape == stack.shape and np.array_equal(stack.grad.numpy(), np.stack(want))
    assert calls[-1] == [True, True, True]
    # an fp16-stored prediction gets its gradient in its own dtype: the float32 gradient of its exact up-conversion, rounded
    half = [_t(p.astype(np.float16)).requires_grad_(True) for p in preds]
    ofl.flow_sequence_loss(half, _t(gt), tm, max_flow=6.0, penalty=penalty, normalise=normalise).backward(_t(g))
    want16 = so.grads([p.astype(np.float16) for p in preds], gt, mask, 6.0, penalty, normalise, 0.8, g)
    for i in range(t):
        assert half[i].grad.dtype == torch.float16 and np.array_equal(half[i].grad.numpy(), want16[i].astype(np.float16))
    # 3-D predictions get 3-D gradients
    one = [_t(p[0]).requires_grad_(True) for p in preds]
    ofl.flow_sequence_loss(one, _t(gt[0]), tm[0], max_flow=6.0, penalty=penalty, normalise=normalise).backward(torch.tensor(g[0]))
    want1 = so.grads([p[:1] for p in preds], gt[:1], mask[:1], 6.0, penalty, normalise, 0.8, g[:1])
    for i in range(t):
        assert one[i].grad.shape == (2, h, w) and np.array_equal(one[i].grad.numpy(), want1[i][0])


def test_api_checks_and_their_messages(oracle_native, monkeypatch):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _sequence_loss

    def never(*args, **kw):
        raise AssertionError("the checks come before the kernel")
    for name in ("flow_sequence_loss", "flow_sequence_loss_grad", "sequence_loss", "sequence_stats"):
        monkeypatch.setattr(_sequence_loss, name, never)
    pre = r"Error scoring flow sequence: "
    vec = torch.zeros(2, 2, 5, 7)
    good, gt = ofl.Flow(vec, 't'), ofl.Flow(vec, 't')
    for call in (ofl.Flow.sequence_loss, ofl.Flow.sequence_stats):
        for bad in (good, vec, [vec], "flows", None, [good, vec], (good, 3)):
            with pytest.raises(TypeError, match=pre + "Preds needs to be a list or a tuple of flow objects"):
                call(bad, gt)
        for bad in (vec, None, [good]):
            with pytest.raises(TypeError, match=pre + "Gt needs to be of type 'Flow'"):
                call([good], bad)
        for bad in ([], [good] * 33):
            with pytest.raises(ValueError, match=pre + "The sequence needs to hold 1 to 32 predictions"):
                call(bad, gt)
        for bad in (ofl.Flow(torch.zeros(1, 2, 5, 7), 't'), ofl.Flow(torch.zeros(2, 2, 7, 5), 't'), ofl.Flow(torch.zeros(2, 5, 7), 't')):
            with pytest.raises(ValueError, match=pre + "Flow fields need to have the same shape"):
                call([good, bad], gt)
            with pytest.raises(ValueError, match=pre + "Flow fields need to have the same shape"):
                call([good], bad)
        with pytest.raises(ValueError, match=pre + "Flow fields need to have the same reference"):
            call([good, ofl.Flow(vec, 's')], gt)
        for bad in ("0.8", None.__class__, [0.8], True):
            with pytest.raises(TypeError, match=pre + "Gamma needs to be an integer or a float"):
                call([good], gt, gamma=bad)
            with pytest.raises(TypeError, match=pre + "Max_flow needs to be an integer or a float"):
                call([good], gt, max_flow=bad)
        for bad in (0, -0.5, math.inf, math.nan):
            with pytest.raises(ValueError, match=pre + "Gamma needs to be finite and larger than 0"):
                call([good], gt, gamma=bad)
        for bad in (0, -1.0, math.nan, -math.inf):
            with pytest.raises(ValueError, match=pre + "Max_flow needs to be larger than 0"):
                call([good], gt, max_flow=bad)
        for bad in ('L1', 'huber', 1, ['l1']):
            with pytest.raises(ValueError, match=pre + "Penalty needs to be 'l1' or 'l2'"):
                call([good], gt, penalty=bad)
        for bad in ('ALL', 'mean', 0, ['all']):
            with pytest.raises(ValueError, match=pre + "Normalise needs to be 'all' or 'valid'"):
                call([good], gt, normalise=bad)
        for bad in (1, 0, "True"):
            with pytest.raises(TypeError, match=pre + "Consider_mask needs to be boolean"):
                call([good], gt, consider_mask=bad)
    call = ofl.flow_sequence_loss
    for bad in ("flows", None, [vec, 3], [good]):
        with pytest.raises(TypeError, match=pre + "Flows needs to be a list or a tuple of tensors"):
            call(bad, vec)
    for bad in ([vec.double()], [vec, vec.to(torch.bfloat16)], vec.long()[None]):
        with pytest.raises(TypeError, match=pre + "Flows need to be of dtype float32 or float16"):
            call(bad, vec)
    for bad in ([], [vec] * 33, torch.zeros(33, 2, 5, 7)):
        with pytest.raises(ValueError, match=pre + "The sequence needs to hold 1 to 32 predictions"):
            call(bad, vec)
    for bad in (torch.zeros(5, 7), torch.zeros(2, 2, 2, 2, 5, 7)):
        with pytest.raises(ValueError, match=pre + "A stacked tensor of predictions needs to have 4 or 5 dimensions"):
            call(bad, vec)
    for bad in ([torch.zeros(5, 7)], [torch.zeros(2, 3, 5, 7)], [torch.zeros(3, 5, 7)], [torch.zeros(2, 2, 0, 7)]):
        with pytest.raises(ValueError, match=pre + "Flows need to be of shape 2-H-W or N-2-H-W"):
            call(bad, vec)
    with pytest.raises(ValueError, match=pre + "Flows need to have the same shape"):
        call([vec, vec[:1]], vec)
    for bad in (vec[:1], torch.zeros(2, 2, 7, 5), vec[0]):
        with pytest.raises(ValueError, match=pre + "Gt needs to have the shape of the flows"):
            call([vec], bad)
    with pytest.raises(ValueError, match=pre + "Penalty"):
        call([vec], vec, penalty='l3')
    with pytest.raises(TypeError, match=pre + "Gamma"):
        call([vec], vec, gamma='0.8')
    assert (_sequence_loss.MAX_T, _sequence_loss.CHUNK, _sequence_loss.record_length(12)) == (32, so.CHUNK, 28)
    assert _sequence_loss.weights_of(3, 0.5) == [0.25, 0.5, 1.0] == so.weights(3, 0.5)


def test_the_methods_and_the_wrapper_are_exported():
    import oflibpytorch_amd as ofl
    assert callable(ofl.Flow.sequence_loss) and callable(ofl.Flow.sequence_stats) and callable(ofl.flow_sequence_loss)
    assert isinstance(ofl.Flow.__dict__['sequence_loss'], staticmethod) and isinstance(ofl.Flow.__dict__['sequence_stats'], staticmethod)
    doc = " ".join(ofl.Flow.sequence_loss.__doc__.split())
    assert "masks of the predictions are NOT read" in doc
    assert "strictly" in " ".join(ofl.Flow.sequence_stats.__doc__.split())
    assert "sequence_loss" in ofl.__doc__ and "flow_sequence_loss" in ofl.__doc__


# ---- the C ABI: declared, exported, and every rejected argument is rejected before any launch -----------------------------------------
def test_c_abi_declarations_and_argument_checks_need_no_gpu():
    from oflibpytorch_amd import _native, _sequence_loss
    names = {"ofl_flow_sequence_loss_workspace_bytes", "ofl_flow_sequence_loss_f64", "ofl_flow_sequence_loss_grad_f32"}
    assert names <= set(_native.exported_symbols())
    header = open(_native._build.HEADERS[0]).read()
    for name in names:
        assert (" %s(" % name) in header
    assert "#define OFL_SEQUENCE_LOSS_CHUNK %d\n" % so.CHUNK in header and "#define OFL_SEQUENCE_LOSS_MAX_T %d\n" % so.MAX_T in header
    assert any(src.endswith("ofl_sequence_loss.hip") for src in _native._build.SOURCES)
    lib = _sequence_loss._library()
    for name in names:
        assert hasattr(lib, name)                                        # present in the built library
    assert lib.ofl_version() == _native.ABI_VERSION == 36                # names were added, no signature changed
    E_NULL, E_SHAPE, E_ARG = -1, -2, -3
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(4096)               # never dereferenced: every call below is rejected first
    odd, odd8 = ctypes.c_void_p(4098), ctypes.c_void_p(4100)

    def arrays(t, ptr=4096, bs=0, half=0):
        t = max(t, 1)
        return (ctypes.c_void_p * t)(*[ptr] * t), (ctypes.c_int64 * t)(*[bs] * t), (ctypes.c_int32 * t)(*[half] * t)

    def fwd(t=3, ptr=4096, bs=0, half=0, preds=None, gt=one, gt_bs=0, gt_half=0, mask=one, mask_bs=0, max_flow=400.0, penalty=0, normalise=0,
            ws=one, rec=one, n=1, h=4, w=4):
        p, s, k = arrays(min(t, 40), ptr, bs, half)
        return lib.ofl_flow_sequence_loss_f64(p if preds is None else preds, s, k, t, gt, gt_bs, gt_half, mask, mask_bs, max_flow, penalty,
                                              normalise, ws, rec, n, h, w, null)

    def bwd(t=3, ptr=4096, bs=0, half=0, preds=None, gt=one, gt_bs=0, gt_half=0, mask=one, mask_bs=0, max_flow=400.0, penalty=0, normalise=0,
            scale=one, grads=4096, n=1, h=4, w=4):
        p, s, k = arrays(min(t, 40), ptr, bs, half)
        g = null if grads is None else (ctypes.c_void_p * max(min(t, 40), 1))(*[grads] * max(min(t, 40), 1))
        return lib.ofl_flow_sequence_loss_grad_f32(p if preds is None else preds, s, k, t, gt, gt_bs, gt_half, mask, mask_bs, max_flow,
                                                   penalty, normalise, scale, g, n, h, w, null)
    shared = ((dict(preds=null), E_NULL), (dict(gt=null), E_NULL), (dict(ptr=None), E_NULL),
              (dict(t=0), E_SHAPE), (dict(t=33), E_SHAPE), (dict(t=-1), E_SHAPE), (dict(n=0), E_SHAPE), (dict(n=65536), E_SHAPE),
              (dict(h=0), E_SHAPE), (dict(w=-1), E_SHAPE), (dict(h=65536, w=32768), E_SHAPE),
              (dict(penalty=2), E_ARG), (dict(penalty=-1), E_ARG), (dict(normalise=2), E_ARG), (dict(normalise=-1), E_ARG),
              (dict(max_flow=0.0), E_ARG), (dict(max_flow=-1.0), E_ARG), (dict(max_flow=math.nan), E_ARG),
              (dict(half=2), E_ARG), (dict(gt_half=-1), E_ARG), (dict(bs=-4), E_ARG), (dict(gt_bs=-1), E_ARG), (dict(mask_bs=-1), E_ARG),
              (dict(ptr=4098), E_ARG), (dict(gt=odd), E_ARG))
    for kw, code in shared + ((dict(ws=null), E_NULL), (dict(rec=null), E_NULL), (dict(ws=odd8), E_ARG), (dict(rec=odd8), E_ARG)):
        assert fwd(**kw) == code, kw
    for kw, code in shared + ((dict(scale=null), E_NULL), (dict(grads=None), E_NULL), (dict(grads=0), E_NULL), (dict(scale=odd), E_ARG),
                              (dict(grads=4098), E_ARG)):
        assert bwd(**kw) == code, kw
    wsb = lib.ofl_flow_sequence_loss_workspace_bytes
    assert wsb(12, 3, 1, so.CHUNK) == 3 * 28 * 8 and wsb(12, 3, 1, so.CHUNK + 1) == 3 * 2 * 28 * 8 and wsb(1, 1, 1, 1) == 6 * 8
    assert wsb(32, 8, 1080, 1920) == 8 * ((1080 * 1920 + so.CHUNK - 1) // so.CHUNK) * 68 * 8
    for bad in ((0, 1, 4, 4), (33, 1, 4, 4), (3, 0, 4, 4), (3, 65536, 4, 4), (3, 1, 0, 4), (3, 1, 65536, 32768)):
        assert wsb(*bad) == E_SHAPE, bad
