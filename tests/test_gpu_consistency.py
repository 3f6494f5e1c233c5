"""GPU tier of Flow.consistency / consistency_mask / filter_consistent (ofl_consistency.hip) against tests/consistency_oracle.py
(DESIGN.md 3.18): the three maps bit for bit, both counts and the maximum exactly, both float64 sums within count * 2^-52 relative of the
exact sum (the terms are not negative, so this bounds ANY summation order), and the residual against combine_with(mode 3) on the device.

Frames: 2 x 2 (the smallest allowed), 5 x 7 (h w odd: the per-element form), 8 x 12 (h w % 4 == 0: the vector form), 20 x 28, 67 x 131
(9 blocks per image, per-element), 1080 x 1920 (the cap of 256 blocks per image: each loops 7 or 8 times, the finish kernel adds 256
records).  The inputs and what they show are checked on the CPU (tests/test_consistency_host.py)."""
import math

import numpy as np
import pytest
import torch

import consistency_oracle as co

pytestmark = pytest.mark.gpu

REFS = ['s', 't']
# the two smallest frames once more with a tenth of the vectors: at full size nearly every partner of theirs leaves the frame
CASES = [f + (1.0,) for f in co.FRAMES] + [(1, 2, 2, 0.1), (2, 5, 7, 0.1)]


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _flows(n, h, w, ref, scale=1.0, dtype_a=torch.float32, dtype_b=torch.float32, masks=True):
    import oflibpytorch_amd as ofl
    a, back, am, bm = (torch.from_numpy(x.copy()).to(_dev()) for x in co.case(n, h, w, ref, scale))
    return ofl.Flow(a.to(dtype_a), ref, am if masks else None), ofl.Flow(back.to(dtype_b), ref, bm if masks else None)


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint8) if a.dtype == bool else a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(got: dict, want: dict, what=""):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(_bits(got[k].to(torch.float64) if got[k].dtype == torch.int64 else got[k]),
                              _bits(want[k].to(torch.float64) if want[k].dtype == torch.int64 else want[k])), (what, k)


def _raw(a, back, ref, alpha, beta, consider_mask=True, **want):
    from oflibpytorch_amd import _consistency
    return _consistency.flow_consistency(a._fv, back._fv, a._mask if consider_mask else None, back._mask if consider_mask else None,
                                         -1.0 if ref == 's' else 1.0, alpha, beta, **want)


@pytest.mark.parametrize("ref", REFS)
@pytest.mark.parametrize("n,h,w,scale", CASES)
def test_maps_counts_max_and_sums(n, h, w, scale, ref):
    from oflibpytorch_amd import _native
    alpha, beta = co.frame_params(n, h, w)
    want = co.reference(n, h, w, ref, True, scale)
    a, back = _flows(n, h, w, ref, scale)
    res = a.consistency(back, alpha=alpha, beta=beta)
    assert 'flow_consistency_finish_kernel' in _native.last_kernel_name()
    assert res['error'].dtype == torch.float32 and res['error'].shape == (n, h, w) and res['error'].device == a.vecs.device
    assert res['consistent'].dtype == torch.bool and res['known'].dtype == torch.bool
    err = res['error'].cpu().numpy()
    assert np.array_equal(err.view(np.uint32), want['error'].view(np.uint32))            # bit for bit, 0 where not known
    assert np.array_equal(res['known'].cpu().numpy(), want['known']) and np.array_equal(res['consistent'].cpu().numpy(), want['consistent'])
    assert set(np.unique(_bits(res['known']))) <= {0, 1} and set(np.unique(_bits(res['consistent']))) <= {0, 1}
    assert not err[~want['known']].any()
    if scale != 1.0:
        assert want['known'].any() and (h * w == 4 or want['consistent'].any())          # (what this variant is for; 2 x 2 is all noise)
    rec = _raw(a, back, ref, alpha, beta, want_error=False, want_consistent=False, want_known=False)[3].cpu().numpy()
    ref_rec = want['records']
    assert rec.shape == (n, 8) and rec.dtype == np.float64 and not rec[:, 5:].any()
    assert rec[:, 0].tolist() == ref_rec[:, 0].tolist() and rec[:, 1].tolist() == ref_rec[:, 1].tolist()
    assert rec[:, 3].tolist() == ref_rec[:, 3].tolist()
    for i in range(n):
        for slot, cnt in ((2, ref_rec[i, 0]), (4, ref_rec[i, 1])):
            got_sum, exact = rec[i, slot], ref_rec[i, slot]
            print("image %d slot %d: sum %.17g, exact %.17g, relative difference %.3g, bound %.3g" %
                  (i, slot, got_sum, exact, abs(got_sum - exact) / max(exact, 1e-300), cnt * 2.0 ** -52))
            assert abs(got_sum - exact) <= cnt * 2.0 ** -52 * exact
    # the dict: the record, divided
    assert res['count'].dtype == torch.int64 and res['count'].tolist() == ref_rec[:, 0].tolist()
    assert res['consistent_count'].dtype == torch.int64 and res['consistent_count'].tolist() == ref_rec[:, 1].tolist()
    with np.errstate(all='ignore'):
        for key, num, den in (('rate', 1, 0), ('mean_error', 2, 0), ('mean_error_consistent', 4, 1)):
            assert res[key].dtype == torch.float64
            assert np.array_equal(res[key].cpu().numpy(), rec[:, num] / rec[:, den], equal_nan=True), key
    assert res['max_error'].tolist() == ref_rec[:, 3].tolist()


@pytest.mark.parametrize("ref", REFS)
@pytest.mark.parametrize("n,h,w,scale", CASES)
def test_residual_and_known_are_mode_3_of_the_device(n, h, w, scale, ref):
    """On known pixels `error` is np.sqrt (float32) of the squared vectors of combine_with(..., 3) as the package computes it on the
    device; `known` is that result's mask."""
    alpha, beta = co.frame_params(n, h, w)
    a, back = _flows(n, h, w, ref, scale)
    comb = a.combine_with(back, 3) if ref == 's' else back.combine_with(a, 3)
    res = a.consistency(back, alpha=alpha, beta=beta)
    mask = comb.mask.cpu().numpy()
    v = comb.vecs.cpu().numpy()
    e = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1])
    assert e.dtype == np.float32
    assert np.array_equal(res['known'].cpu().numpy(), mask)
    err = res['error'].cpu().numpy()
    assert np.array_equal(err[mask].view(np.uint32), e[mask].view(np.uint32)) and not err[~mask].any()


def test_defaults_are_alpha_001_beta_05():
    n, h, w = 2, 20, 28
    for ref in REFS:
        a, back = _flows(n, h, w, ref)
        want = co.check(*co.case(n, h, w, ref), ref, 0.01, 0.5)
        res = a.consistency(back)
        assert np.array_equal(res['consistent'].cpu().numpy(), want['consistent'])
        assert want['consistent'].sum() > co.reference(n, h, w, ref)['consistent'].sum()       # (the table's beta is tighter)
        _same(res, a.consistency(back, alpha=0.01, beta=0.5))


def test_the_bound_is_inclusive():
    """a = (1, 0), back = 0: e^2 = 1, m2 = 1; alpha = 0.25 and beta = 0.75 put the bound at exactly 1, the float32 before 0.75 below it."""
    import oflibpytorch_amd as ofl
    a = torch.zeros(1, 2, 6, 8, device=_dev())
    a[:, 0] = 1.0
    fa, fb = ofl.Flow(a, 's'), ofl.Flow(torch.zeros_like(a), 's')
    res = fa.consistency(fb, alpha=0.25, beta=0.75)
    inside = torch.zeros(1, 6, 8, dtype=torch.bool, device=_dev())
    inside[:, :, :7] = True
    assert torch.equal(res['known'], inside) and torch.equal(res['consistent'], inside)
    assert res['error'][inside].tolist() == [1.0] * 42 and res['rate'].tolist() == [1.0]
    res = fa.consistency(fb, alpha=0.25, beta=0.75 - 2.0 ** -24)
    assert torch.equal(res['known'], inside) and not bool(res['consistent'].any()) and res['consistent_count'].tolist() == [0]
    assert res['count'].tolist() == [42] and res['mean_error'].tolist() == [1.0] and res['max_error'].tolist() == [1.0]
    assert bool(torch.isnan(res['mean_error_consistent']).all())


@pytest.mark.parametrize("ref", REFS)
@pytest.mark.parametrize("n,h,w", [(2, 5, 7), (3, 8, 12), (2, 67, 131)])
def test_consider_mask_false_reads_no_mask(n, h, w, ref):
    import oflibpytorch_amd as ofl
    alpha, beta = co.frame_params(n, h, w)
    want = co.reference(n, h, w, ref, False)
    a, back = _flows(n, h, w, ref)
    none = torch.zeros(n, h, w, dtype=torch.bool, device=_dev())
    blind_a, blind_b = ofl.Flow(a.vecs, ref, none), ofl.Flow(back.vecs, ref, none.clone())
    plain_a, plain_b = _flows(n, h, w, ref, masks=False)
    got = a.consistency(back, alpha=alpha, beta=beta, consider_mask=False)
    assert np.array_equal(got['error'].cpu().numpy().view(np.uint32), want['error'].view(np.uint32))
    assert np.array_equal(got['known'].cpu().numpy(), want['known']) and np.array_equal(got['consistent'].cpu().numpy(), want['consistent'])
    assert got['count'].tolist() == want['records'][:, 0].tolist()
    _same(blind_a.consistency(blind_b, alpha=alpha, beta=beta, consider_mask=False), got, "masks of False")
    _same(plain_a.consistency(plain_b, alpha=alpha, beta=beta), got, "no masks")
    assert not bool(blind_a.consistency(blind_b, alpha=alpha, beta=beta)['known'].any())        # ... and with them, nothing is known


@pytest.mark.parametrize("ref", REFS)
@pytest.mark.parametrize("n,h,w", [(2, 5, 7), (3, 8, 12), (2, 67, 131)])
def test_fp16_stored_flows_give_the_bits_of_their_float_copies(n, h, w, ref):
    alpha, beta = co.frame_params(n, h, w)
    h16 = torch.float16
    for da, db in ((h16, torch.float32), (torch.float32, h16), (h16, h16)):
        a, back = _flows(n, h, w, ref, dtype_a=da, dtype_b=db)
        assert a._fv.dtype == da and back._fv.dtype == db                                   # read as stored: no float copy is made
        import oflibpytorch_amd as ofl
        fa, fb = ofl.Flow(a._fv.float(), ref, a.mask), ofl.Flow(back._fv.float(), ref, back.mask)
        want = fa.consistency(fb, alpha=alpha, beta=beta)
        _same(a.consistency(back, alpha=alpha, beta=beta), want, str((da, db)))
        assert a._fv.dtype == da and back._fv.dtype == db
        assert bool(want['known'].any())
        oracle = co.check(a._fv.cpu().numpy(), back._fv.cpu().numpy(), a.mask.cpu().numpy(), back.mask.cpu().numpy(), ref, alpha, beta)
        assert np.array_equal(want['error'].cpu().numpy().view(np.uint32), oracle['error'].view(np.uint32))


@pytest.mark.parametrize("ref", REFS)
@pytest.mark.parametrize("n,h,w", [(3, 8, 12), (2, 67, 131)])
def test_an_image_has_the_same_bits_alone_in_any_batch_and_on_any_run(n, h, w, ref):
    alpha, beta = co.frame_params(n, h, w)
    a, back = _flows(n, h, w, ref)
    whole = _raw(a, back, ref, alpha, beta)
    again = _raw(a, back, ref, alpha, beta)
    for x, y in zip(whole, again):
        assert np.array_equal(_bits(x), _bits(y))
    for k in range(n):
        for _ in range(2):
            one = _raw(a.select(k), back.select(k), ref, alpha, beta)
            for x, y in zip(whole, one):
                assert np.array_equal(_bits(x[k:k + 1]), _bits(y))


@pytest.mark.parametrize("ref", REFS)
@pytest.mark.parametrize("n,h,w", [(2, 5, 7), (3, 8, 12), (2, 67, 131)])
def test_consistency_mask_and_filter_consistent(n, h, w, ref):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _native
    alpha, beta = co.frame_params(n, h, w)
    a, back = _flows(n, h, w, ref)
    cons = a.consistency(back, alpha=alpha, beta=beta)['consistent']
    only = a.consistency_mask(back, alpha=alpha, beta=beta)
    name = _native.last_kernel_name()
    assert 'flow_consistency_kernel' in name and 'finish' not in name                      # one launch: no record, no second kernel
    assert only.dtype == torch.bool and torch.equal(only, cons) and set(np.unique(_bits(only))) <= {0, 1}
    vecs_before, mask_before = a.vecs.clone(), a.mask.clone()
    f = a.filter_consistent(back, alpha=alpha, beta=beta)
    assert f.ref == ref and f.vecs.data_ptr() == a.vecs.data_ptr() and torch.equal(f.vecs, vecs_before)
    assert torch.equal(a.mask, mask_before) and torch.equal(f.mask, mask_before & cons)
    # ... and it is a flow like any other: a further apply gives what the same vectors under the same mask give
    img = torch.rand(n, 3, h, w, device=_dev())
    got = f.apply(img, return_valid_area=True)
    want = ofl.Flow(vecs_before, ref, mask_before & cons).apply(img, return_valid_area=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    if n == 3:                                                                           # a flow all of whose known vectors are filtered away
        none = a.filter_consistent(back, alpha=0, beta=0)
        assert torch.equal(none.mask, mask_before & a.consistency_mask(back, alpha=0, beta=0))
        assert none.is_zero(masked=True).tolist() == ofl.Flow(vecs_before, ref, none.mask).is_zero(masked=True).tolist()


def _partner_taps(a, ref, h, w):
    """The integer taps (y0, y1, x0, x1) of every pixel's partner, in the kernel's float32 steps (NumPy restates unnormalise())."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    sign = np.float32(-1.0 if ref == 's' else 1.0)

    def pos(grid, flow, size):
        g = (grid - sign * flow) * np.float32(2.0)
        g = g / np.float32(size - 1)
        g = g - np.float32(1.0)
        return (g + np.float32(1.0)) * (np.float32(size - 1) / np.float32(2.0))
    sx, sy = pos(x, a[:, 0], w), pos(y, a[:, 1], h)
    return np.floor(sy), np.floor(sy) + 1, np.floor(sx), np.floor(sx) + 1


@pytest.mark.parametrize("ref", REFS)
def test_non_finite_vectors(ref):
    """No validation pass runs and none is needed: a NaN or an inf in `a` fails the comparisons of its own pixel, which is unknown, and
    touches no other.  `known` never reads back's vectors (it is the mask of mode 3): a NaN in `back` leaves it as it is and makes
    the error NaN, and the pixel inconsistent, exactly where one of the partner's taps inside the frame is that vector -- whatever
    the tap's weight, as 0 * NaN is NaN in the blend of the backward warp too."""
    n, h, w = 2, 20, 28
    alpha, beta = co.frame_params(n, h, w)
    a, back = _flows(n, h, w, ref, scale=0.5)
    clean = a.consistency(back, alpha=alpha, beta=beta)
    known = clean['known'].cpu().numpy()
    where = [np.argwhere(known[i]) for i in range(n)]
    assert all(len(x) >= 20 for x in where)
    picks = [(0, 1, float('nan'), 0), (0, 3, float('inf'), 1), (1, 2, -float('inf'), 0), (1, 4, float('nan'), 1)]
    spots = [(i, int(where[i][len(where[i]) * k // 5][0]), int(where[i][len(where[i]) * k // 5][1]), value, c) for i, k, value, c in picks]
    bad_vecs = a.vecs.clone()
    for i, y, x, value, c in spots:
        bad_vecs[i, c, y, x] = value
    import oflibpytorch_amd as ofl
    bad = ofl.Flow._wrap(bad_vecs, ref, a.mask)                                           # (the constructor would refuse it)
    got = bad.consistency(back, alpha=alpha, beta=beta)
    want_known = known.copy()
    for i, y, x, _, _ in spots:
        want_known[i, y, x] = False
    assert np.array_equal(got['known'].cpu().numpy(), want_known)
    assert np.array_equal(got['consistent'].cpu().numpy(), clean['consistent'].cpu().numpy() & want_known)
    want_err = clean['error'].cpu().numpy().copy()
    want_err[~want_known] = 0.0
    assert np.array_equal(got['error'].cpu().numpy().view(np.uint32), want_err.view(np.uint32))
    assert got['count'].tolist() == want_known.reshape(n, -1).sum(1).tolist()
    assert bool(torch.isfinite(got['mean_error']).all()) and bool(torch.isfinite(got['max_error']).all())
    # a NaN in back
    y0, y1, x0, x1 = _partner_taps(a.vecs.cpu().numpy(), ref, h, w)
    i = 1
    py, px = where[i][len(where[i]) // 2]                                                 # a known pixel: its partner's first tap gets the NaN
    yn, xn = int(y0[i, py, px]), int(x0[i, py, px])
    bad_back = back.vecs.clone()
    bad_back[i, 0, yn, xn] = float('nan')
    got = a.consistency(ofl.Flow._wrap(bad_back, ref, back.mask), alpha=alpha, beta=beta)
    hit = np.zeros((n, h, w), bool)
    hit[i] = (((y0 == yn) | (y1 == yn)) & ((x0 == xn) | (x1 == xn)))[i]
    assert hit[i, py, px] and 1 <= (hit & known).sum() <= 6
    assert np.array_equal(got['known'].cpu().numpy(), known)
    err, cons = got['error'].cpu().numpy(), got['consistent'].cpu().numpy()
    assert np.isnan(err[hit & known]).all() and not cons[hit].any()
    rest = ~(hit & known)
    assert np.array_equal(err[rest].view(np.uint32), clean['error'].cpu().numpy()[rest].view(np.uint32))
    assert np.array_equal(cons[rest], clean['consistent'].cpu().numpy()[rest])
    assert got['count'].tolist() == clean['count'].tolist()
    assert got['max_error'].tolist() == [float(clean['error'].cpu().numpy()[k][(known & rest)[k]].max()) for k in range(n)]
    assert math.isnan(float(got['mean_error'][i])) and float(got['mean_error'][0]) == float(clean['mean_error'][0])


def test_an_image_without_a_known_pixel():
    import oflibpytorch_amd as ofl
    n, h, w = 3, 8, 12
    a, back = _flows(n, h, w, 's')
    far = a.vecs.clone()
    far[1, 0] += 50.0                                                                    # every partner of image 1 leaves the frame
    res = ofl.Flow(far, 's', a.mask).consistency(back, beta=0.1)
    assert res['count'][1].item() == 0 and res['consistent_count'][1].item() == 0 and res['max_error'][1].item() == 0.0
    for k in ('rate', 'mean_error', 'mean_error_consistent'):
        assert math.isnan(res[k][1].item()) and math.isfinite(res[k][0].item()) and math.isfinite(res[k][2].item()), k
    assert not bool(res['known'][1].any()) and not bool(res['error'][1].any()) and not bool(res['consistent'][1].any())
    want = co.reference(n, h, w, 's')
    for i in (0, 2):
        assert np.array_equal(res['error'][i].cpu().numpy().view(np.uint32), want['error'][i].view(np.uint32))
        assert res['count'][i].item() == want['records'][i, 0]


def test_flow_consistency_adapter_on_tensors_and_arrays():
    import oflibpytorch_amd as ofl
    n, h, w, ref = 2, 20, 28, 't'
    a, back, am, bm = co.case(n, h, w, ref)
    fa, fb = _flows(n, h, w, ref)
    want = fa.consistency(fb, beta=0.1)
    got = ofl.flow_consistency(a.copy(), back.copy(), ref, am.copy(), bm.copy(), beta=0.1)                 # ndarrays
    assert all(isinstance(v, torch.Tensor) for v in got.values())
    _same({k: v.to(_dev()) for k, v in got.items()}, want, "ndarrays")
    dev = [torch.from_numpy(x.copy()).to(_dev()) for x in (a, back, am, bm)]
    got = ofl.flow_consistency(dev[0], dev[1], ref, dev[2], dev[3], beta=0.1)                              # tensors on the device
    assert got['error'].device == dev[0].device
    _same(got, want, "tensors")
    one = ofl.flow_consistency(dev[0][1], dev[1][1], ref, dev[2][1], dev[3][1], beta=0.1)                  # 3-D in: no batch dimension out
    assert one['error'].shape == (h, w) and one['consistent'].shape == (h, w) and one['count'].shape == () and one['rate'].shape == ()
    _same({k: v.unsqueeze(0) for k, v in one.items()}, {k: v[1:2] for k, v in want.items()}, "3-D")


@pytest.mark.parametrize("ref", REFS)
def test_offset_views_take_the_per_element_form_and_give_the_same_bits(ref):
    """Tensors that start 4 bytes (fp16: 2 bytes) into their storage: 16-byte loads of `a` are not aligned there, and the launch
    takes the per-element form; `back` is read one element at a time in either form.  Same bits whichever operand is offset."""
    import oflibpytorch_amd as ofl
    n, h, w = 3, 8, 12                                                                   # h w % 4 == 0: aligned operands take the vector form
    alpha, beta = co.frame_params(n, h, w)
    a, back = _flows(n, h, w, ref)
    want = a.consistency(back, alpha=alpha, beta=beta)

    def offset(t):
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        view = flat[1:].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % 16 != 0 and view.data_ptr() == flat.data_ptr() + t.element_size()
        return view
    for off_a, off_b, off_m in ((False, True, False), (True, False, False), (True, True, True), (False, False, True)):
        fa = ofl.Flow(offset(a.vecs) if off_a else a.vecs, ref, offset(a.mask) if off_m else a.mask)
        fb = ofl.Flow(offset(back.vecs) if off_b else back.vecs, ref, offset(back.mask) if off_m else back.mask)
        assert fa.vecs.data_ptr() % 16 == (4 if off_a else 0) and fb.vecs.data_ptr() % 16 == (4 if off_b else 0)
        _same(fa.consistency(fb, alpha=alpha, beta=beta), want, str((off_a, off_b, off_m)))
        assert torch.equal(fa.consistency_mask(fb, alpha=alpha, beta=beta), want['consistent'])
    ha, hb = _flows(n, h, w, ref, dtype_a=torch.float16, dtype_b=torch.float16)
    want16 = ha.consistency(hb, alpha=alpha, beta=beta)
    fa, fb = ofl.Flow(offset(ha._fv), ref, a.mask), ofl.Flow(offset(hb._fv), ref, back.mask)
    assert fa._fv.dtype == torch.float16 and fa._fv.data_ptr() % 8 == 2
    _same(fa.consistency(fb, alpha=alpha, beta=beta), want16, "fp16")


def test_back_on_another_device_is_moved_and_nothing_is_differentiable():
    import oflibpytorch_amd as ofl
    n, h, w, ref = 2, 20, 28, 's'
    a, back = _flows(n, h, w, ref)
    want = a.consistency(back, beta=0.1)
    cpu_back = ofl.Flow(back.vecs.cpu(), ref, back.mask.cpu())
    assert cpu_back.device.type == 'cpu'
    _same(a.consistency(cpu_back, beta=0.1), want, "back on the CPU")
    va = a.vecs.clone().requires_grad_(True)
    res = ofl.Flow(va, ref, a.mask).consistency(back, beta=0.1)
    assert not res['error'].requires_grad and not res['mean_error'].requires_grad
    _same(res, want, "requires_grad")
