"""CPU tier of Flow.consistency / consistency_mask / filter_consistent: the oracle (tests/consistency_oracle.py) on
cases written out by hand and against the oracle's combine_with(mode 3), the inputs the GPU tier runs on, the host logic of the API with
the native call served by the oracle, and the C ABI's argument checks.  No device."""
import ctypes
import math

import numpy as np
import pytest
import torch

import consistency_oracle as co
from oracle import oracle

BIG = [f for f in co.FRAMES if f[1] >= 8 and f[2] >= 8]


@pytest.fixture
def consistency_native(oracle_native, monkeypatch):
    from oflibpytorch_amd import _consistency
    monkeypatch.setattr(_consistency, "flow_consistency", co.fake_flow_consistency)
    return _consistency


def _const(u, v, n=1, h=6, w=7):
    a = np.empty((n, 2, h, w), np.float32)
    a[:, 0], a[:, 1] = u, v
    return a


# ---- the oracle on hand-computed cases ---------------------------------------------------------------------------------------
def test_the_bound_is_inclusive():
    """a = (1, 0), back = 0: e^2 = 1 and m2 = 1 wherever the partner is inside; alpha = 0.25, beta = 0.75 make the bound exactly 1."""
    a, back = _const(1, 0), _const(0, 0)
    r = co.check(a, back, None, None, 's', 0.25, 0.75)
    inside = np.zeros((1, 6, 7), bool)
    inside[:, :, :6] = True                                  # the partner of column 6 is column 7: outside
    assert np.array_equal(r['known'], inside)
    assert r['error'][inside].tolist() == [1.0] * 36 and not r['error'][~inside].any()
    assert np.array_equal(r['consistent'], inside)
    below = 0.75 - 2.0 ** -24                                # the float32 before 0.75: 0.25 + it is the float32 before 1
    assert np.float32(below) == below and np.float32(0.25) + np.float32(below) < np.float32(1.0)
    r = co.check(a, back, None, None, 's', 0.25, below)
    assert np.array_equal(r['known'], inside) and not r['consistent'].any()
    assert r['records'].tolist() == [[36, 0, 36, 1, 0, 0, 0, 0]]


@pytest.mark.parametrize("ref,u,v,xs,ys", [
    # (w = 5, h = 4) 's': the partner of (x, y) is (x + u, y + v); 't': (x - u, y - v).  Known columns / rows written out by hand
    ('s', 2, 1, [0, 1, 2], [0, 1, 2]), ('t', 2, 1, [2, 3, 4], [1, 2, 3]),
    ('s', -1, 0, [1, 2, 3, 4], [0, 1, 2, 3]), ('t', -1, 0, [0, 1, 2, 3], [0, 1, 2, 3]),
    ('s', 0, -3, [0, 1, 2, 3, 4], [3]), ('t', 0, -3, [0, 1, 2, 3, 4], [0]),
    ('s', 4, 3, [0], [0]), ('t', 4, 3, [4], [3]),
    ('s', 5, 0, [], []), ('t', 0, 4, [], []), ('s', -7, 2, [], []), ('t', 100, -100, [], []),
])
def test_known_sets_of_integer_translations(ref, u, v, xs, ys):
    a = _const(u, v, 2, 4, 5)
    want = np.zeros((2, 4, 5), bool)
    for y in ys:
        want[:, y, xs] = True
    r = co.check(a, -a, None, None, ref)
    assert np.array_equal(r['known'], want)
    assert not r['error'].any() and np.array_equal(r['consistent'], want)        # back = -a: the round trip closes exactly
    assert r['records'][:, 0].tolist() == [len(xs) * len(ys)] * 2 and r['records'][:, 3].tolist() == [0.0, 0.0]
    # a's mask switches single pixels off, back's mask the pixels whose partner it covers
    am = np.ones((2, 4, 5), bool)
    am[:, 1, 2] = False
    assert np.array_equal(co.check(a, -a, am, None, ref)['known'], want & am)
    if xs:
        bm = np.ones((2, 4, 5), bool)
        sgn = 1 if ref == 's' else -1
        px, py = xs[0] + sgn * u, ys[0] + sgn * v                    # the partner of the first known pixel
        bm[:, py, px] = False
        off = want.copy()
        off[:, ys[0], xs[0]] = False
        assert np.array_equal(co.check(a, -a, None, bm, ref)['known'], off)


@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("n,h,w", [(2, 5, 7), (3, 8, 12), (2, 20, 28), (2, 67, 131)])
def test_residual_and_known_are_mode_3_bit_for_bit(n, h, w, ref):
    a, back, am, bm = co.case(n, h, w, ref)
    r = co.reference(n, h, w, ref)
    if ref == 's':
        vecs, mask, _ = oracle.combine_with(a, am, back, bm, 3, 's')
    else:
        vecs, mask, _ = oracle.combine_with(back, bm, a, am, 3, 't')
    assert np.array_equal(r['du'].view(np.uint32), vecs[:, 0].view(np.uint32))
    assert np.array_equal(r['dv'].view(np.uint32), vecs[:, 1].view(np.uint32))
    assert np.array_equal(r['known'], mask)
    e = np.sqrt(vecs[:, 0] * vecs[:, 0] + vecs[:, 1] * vecs[:, 1])
    assert np.array_equal(r['error'][mask].view(np.uint32), e[mask].view(np.uint32)) and not r['error'][~mask].any()


@pytest.mark.parametrize("ref", ['s', 't'])
@pytest.mark.parametrize("n,h,w", BIG)
def test_the_inputs_show_every_category(n, h, w, ref):
    """A condition on the inputs of the GPU tier, not a tolerance: at least 5 % of the pixels of every frame of 8 x 8 and more are
    known and consistent, known and inconsistent, unknown because the partner leaves the frame, unknown because of a mask."""
    shares = co.categories(n, h, w, ref)
    print(shares)
    assert sorted(shares) == ['consistent', 'inconsistent', 'leaves_frame', 'masked']
    for name, share in shares.items():
        assert share >= 0.05, (name, shares)


def test_the_input_recipe():
    assert len(BIG) == 4 and co.FRAMES == [(1, 2, 2), (2, 5, 7), (3, 8, 12), (2, 20, 28), (2, 67, 131), (1, 1080, 1920)]
    for ref, s in (('s', 1.0), ('t', -1.0)):
        a, back, am, bm = co.case(2, 67, 131, ref)
        assert a.dtype == np.float32 and back.dtype == np.float32 and am.dtype == bool and bm.dtype == bool
        assert not a.flags.writeable and co.case(2, 67, 131, ref)[0] is a                   # computed once, shared, read-only
        assert a[0, 0, 0, 0] == np.float32(3.3) and a[0, 1, -1, -1] == np.float32(-2.6)       # the translation, where the field is 0
        for d in (np.diff(a, axis=2), np.diff(a, axis=3)):
            assert np.abs(d).max() <= 0.02 * 1.001
        noise = back + a
        band = slice(131 // 3, (2 * 131 + 2) // 3)
        assert not noise[..., :band.start].any() and not noise[..., band.stop:].any()
        assert 1.9 < np.abs(noise[..., band]).max() <= 2.0 + 1e-5
        for m in (am, bm):
            assert 0.7 < m.mean() < 0.9
        assert not np.array_equal(am, bm) and not np.array_equal(a[0], a[1])
        small = co.case(2, 5, 7, ref, 0.1)[0]
        assert np.abs(small).max() < 0.4


def test_oracle_steps_are_float32_and_records_exact():
    a = np.array([0.1, 0.2], np.float32).reshape(1, 2, 1, 1) * np.ones((1, 2, 3, 3), np.float32)
    back = np.zeros_like(a)
    r = co.check(a, back, None, None, 's', 0.0, 100.0)
    x, y = np.float32(0.1), np.float32(0.2)
    want = np.sqrt(np.float32(x * x) + np.float32(y * y))
    assert r['known'][0, 0, 0] and r['error'][0, 0, 0] == want and r['error'].dtype == np.float32
    k = int(r['known'].sum())
    assert k == 4 and r["records"][0].tolist() == [4, 4, 4 * float(want), float(want), 4 * float(want), 0, 0, 0]      # (the last row and column point outside)
    # fsum: 2^30 + 4 x 2^-24 is exact in float64, a float32 running sum would lose every small term
    a = np.zeros((1, 2, 2, 3), np.float32)
    a[0, 0] = [[2.0 ** 30, 0, 0], [2.0 ** -24] * 3]
    a[0, 1, 0, 1] = 2.0 ** -24
    r = co.check(a * 0, a, None, None, 's', 0.0, 1e30)                       # a = 0: the partner of a pixel is the pixel itself
    assert r['known'].all() and r['records'][0, 2] == 2.0 ** 30 + 4 * 2.0 ** -24 and r['records'][0, 3] == 2.0 ** 30
    # fp16 storage is up-converted exactly
    h16 = np.array([1.5, -0.25], np.float16).reshape(1, 2, 1, 1) * np.ones((1, 2, 4, 4), np.float16)
    r16, r32 = co.check(h16, -h16, None, None, 't'), co.check(h16.astype(np.float32), -h16.astype(np.float32), None, None, 't')
    assert np.array_equal(r16['error'], r32['error']) and np.array_equal(r16['known'], r32['known'])
    # an image without a known pixel
    r = co.check(_const(50, 0), _const(0, 0), None, None, 's')
    assert not r['known'].any() and not r['records'].any() and not r['error'].any() and not r['consistent'].any()


# ---- host logic: the API with the native call served by the oracle ---------------------------------------------------------------
def _flows(ref='s', n=2, h=20, w=28, masks=True):
    import oflibpytorch_amd as ofl
    a, back, am, bm = (torch.from_numpy(x.copy()) for x in co.case(n, h, w, ref))
    return ofl.Flow(a, ref, am if masks else None), ofl.Flow(back, ref, bm if masks else None)


@pytest.mark.parametrize("ref", ['s', 't'])
def test_consistency_keys_dtypes_shapes_and_values(consistency_native, ref):
    a, back = _flows(ref)
    res = a.consistency(back)
    assert sorted(res) == ['consistent', 'consistent_count', 'count', 'error', 'known', 'max_error', 'mean_error',
                           'mean_error_consistent', 'rate']
    assert res['error'].dtype == torch.float32 and res['error'].shape == (2, 20, 28)
    for k in ('consistent', 'known'):
        assert res[k].dtype == torch.bool and res[k].shape == (2, 20, 28)
    for k in ('count', 'consistent_count'):
        assert res[k].dtype == torch.int64 and res[k].shape == (2,)
    for k in ('rate', 'mean_error', 'max_error', 'mean_error_consistent'):
        assert res[k].dtype == torch.float64 and res[k].shape == (2,)
    want = co.check(*co.case(2, 20, 28, ref), ref)                      # the defaults: alpha 0.01, beta 0.5
    rec = want['records']
    assert np.array_equal(res['error'].numpy(), want['error']) and np.array_equal(res['consistent'].numpy(), want['consistent'])
    assert np.array_equal(res['known'].numpy(), want['known'])
    assert res['count'].tolist() == rec[:, 0].tolist() and res['consistent_count'].tolist() == rec[:, 1].tolist()
    assert res['rate'].tolist() == (rec[:, 1] / rec[:, 0]).tolist() and res['mean_error'].tolist() == (rec[:, 2] / rec[:, 0]).tolist()
    assert res['max_error'].tolist() == rec[:, 3].tolist() and res['mean_error_consistent'].tolist() == (rec[:, 4] / rec[:, 1]).tolist()
    # explicit parameters reach the kernel; consider_mask=False drops both masks
    tight = a.consistency(back, alpha=0, beta=0.125)
    assert np.array_equal(tight['consistent'].numpy(), co.check(*co.case(2, 20, 28, ref), ref, 0.0, 0.125)['consistent'])
    assert int(tight['consistent_count'].sum()) < int(res['consistent_count'].sum())
    nomask = a.consistency(back, consider_mask=False)
    assert np.array_equal(nomask['known'].numpy(), co.check(*co.case(2, 20, 28, ref)[:2], None, None, ref)['known'])


def test_no_known_pixel_gives_nan_means_and_zero_max(consistency_native):
    import oflibpytorch_amd as ofl
    a = ofl.Flow(torch.from_numpy(_const(50, 0, 2)), 's')
    res = a.consistency(ofl.Flow(torch.from_numpy(_const(-50, 0, 2)), 's'))
    assert res['count'].tolist() == [0, 0] and res['consistent_count'].tolist() == [0, 0] and res['max_error'].tolist() == [0.0, 0.0]
    for k in ('rate', 'mean_error', 'mean_error_consistent'):
        assert bool(torch.isnan(res[k]).all()), k
    assert not res['error'].any() and not res['known'].any() and not res['consistent'].any()


def test_consistency_mask_asks_for_one_output(oracle_native, monkeypatch):
    from oflibpytorch_amd import _consistency
    calls = []

    def spy(*args, **kw):
        calls.append(kw)
        return co.fake_flow_consistency(*args, **kw)
    monkeypatch.setattr(_consistency, "flow_consistency", spy)
    a, back = _flows('t')
    m = a.consistency_mask(back, beta=0.1)
    assert calls == [dict(want_error=False, want_known=False, want_record=False)]
    assert m.dtype == torch.bool and np.array_equal(m.numpy(), co.reference(2, 20, 28, 't')['consistent'])


@pytest.mark.parametrize("masks", [True, False])
def test_filter_consistent_keeps_the_vectors_and_narrows_the_mask(consistency_native, masks):
    a, back = _flows('s', masks=masks)
    f = a.filter_consistent(back, beta=0.1)
    cons = a.consistency_mask(back, beta=0.1)
    assert f.ref == 's' and f.vecs.data_ptr() == a.vecs.data_ptr()
    assert torch.equal(f.mask, a.mask & cons) and bool(cons.any()) and not bool(cons.all())
    assert torch.equal(a.mask, torch.from_numpy(co.case(2, 20, 28, 's')[2].copy())) if masks else bool(a.mask.all())      # untouched
    # usable as a flow: the next call validates it under its own mask
    img = torch.rand(2, 1, 20, 28)
    warped, valid = f.apply(img, return_valid_area=True)
    w2, v2 = type(a)(a.vecs, 's', a.mask & cons).apply(img, return_valid_area=True)
    assert torch.equal(warped, w2) and torch.equal(valid, v2)


def test_flow_consistency_adapter_on_tensors_and_arrays(consistency_native):
    import oflibpytorch_amd as ofl
    a, back, am, bm = co.case(2, 20, 28, 't')
    want = ofl.Flow(torch.from_numpy(a.copy()), 't', torch.from_numpy(am.copy())).consistency(
        ofl.Flow(torch.from_numpy(back.copy()), 't', torch.from_numpy(bm.copy())), beta=0.1)
    got = ofl.flow_consistency(a.copy(), back.copy(), 't', am.copy(), bm.copy(), beta=0.1)              # ndarrays, 4-D
    assert sorted(got) == sorted(want)
    for k in want:
        assert torch.equal(got[k], want[k]) or k.startswith('mean') and torch.allclose(got[k], want[k], rtol=0, atol=0, equal_nan=True), k
    one = ofl.flow_consistency(torch.from_numpy(a[1].copy()), torch.from_numpy(back[1].copy()), 't', torch.from_numpy(am[1].copy()),
                               torch.from_numpy(bm[1].copy()), beta=0.1)                                # tensors, 3-D: no batch dimension out
    assert one['error'].shape == (20, 28) and one['known'].shape == (20, 28) and one['count'].shape == ()
    assert torch.equal(one['error'], want['error'][1]) and one['count'] == want['count'][1]
    hwc = ofl.flow_consistency(np.moveaxis(a[1], 0, -1).copy(), np.moveaxis(back[1], 0, -1).copy(), 't', beta=0.1)   # H-W-2, no masks
    assert hwc['error'].shape == (20, 28) and int(hwc['count']) >= int(one['count'])


# ---- the checks of the API, none of which needs a device -----------------------------------------------------------------------------
def test_api_checks_and_their_messages(oracle_native, monkeypatch):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _consistency

    def never(*args, **kw):
        raise AssertionError("the checks come before the kernel")
    monkeypatch.setattr(_consistency, "flow_consistency", never)
    a, back = _flows('s', 2, 6, 7)
    pre = r"Error checking flow consistency: "
    for call in (a.consistency, a.consistency_mask, a.filter_consistent):
        with pytest.raises(TypeError, match=pre + "Back needs to be of type 'Flow'"):
            call(back.vecs)
        with pytest.raises(ValueError, match=pre + "Flow fields need to have the same shape, including batch size"):
            call(back.select(0))
        with pytest.raises(ValueError, match=pre + "Flow fields need to have the same shape, including batch size"):
            call(ofl.Flow(torch.ones(2, 2, 6, 8), 's'))
        with pytest.raises(ValueError, match=pre + "Flow fields need to have the same reference: switch_ref one of them"):
            call(ofl.Flow(back.vecs, 't'))
        for name, key in (("Alpha", "alpha"), ("Beta", "beta")):
            for bad in (True, "1", [0.1], torch.tensor(0.1), np.ones(1)):
                with pytest.raises(TypeError, match=pre + name + " needs to be an integer or a float"):
                    call(back, **{key: bad})
            for bad in (-1, -1e-9, float('nan'), float('inf'), -float('inf')):
                with pytest.raises(ValueError, match=pre + name + " needs to be finite and not negative"):
                    call(back, **{key: bad})
        for bad in (1, 0, "True", 1.0):
            with pytest.raises(TypeError, match=pre + "Consider_mask needs to be boolean"):
                call(back, consider_mask=bad)
    for shape in ((1, 2, 1, 5), (1, 2, 5, 1), (2, 2, 1, 1)):
        thin = ofl.Flow(torch.ones(shape), 't')
        with pytest.raises(ValueError, match=pre + "Flow fields need to be at least 2 pixels high and wide"):
            thin.consistency(ofl.Flow(-torch.ones(shape), 't'))
    # the order: type, shape, reference, size, alpha, beta, consider_mask
    with pytest.raises(ValueError, match="same shape"):
        a.consistency(ofl.Flow(torch.ones(1, 2, 3, 3), 't'), alpha="x", consider_mask=1)
    with pytest.raises(TypeError, match="Alpha"):
        a.consistency(back, alpha="x", beta=-1, consider_mask=1)
    with pytest.raises(ValueError, match="Beta"):
        a.consistency(back, alpha=1, beta=-1, consider_mask=1)
    with pytest.raises(ValueError, match=pre):
        ofl.flow_consistency(a.vecs, back.vecs, 's', alpha=-1)
    with pytest.raises(ValueError, match="Error setting flow reference"):
        ofl.flow_consistency(a.vecs, back.vecs, 'x')


def test_integers_and_zero_are_valid_parameters(consistency_native):
    a, back = _flows('s', 2, 6, 7)
    for alpha, beta in ((0, 0), (1, 2), (0.0, 1e30)):
        res = a.consistency(back, alpha=alpha, beta=beta)
        want = co.check(*co.case(2, 6, 7, 's'), 's', alpha, beta)
        assert np.array_equal(res['consistent'].numpy(), want['consistent'])


# ---- the C ABI: declared, exported, and every rejected argument is rejected before any launch --------------------------------------
def test_c_abi_argument_checks_need_no_gpu():
    from oflibpytorch_amd import _consistency, _native
    assert {"ofl_flow_consistency_workspace_bytes", "ofl_flow_consistency_f32"} <= set(_native.exported_symbols())
    lib = _consistency._library()
    assert lib.ofl_version() == _native.ABI_VERSION == 36               # names were added, no signature changed
    ws = lib.ofl_flow_consistency_workspace_bytes
    assert ws(1, 2, 2) == 64 and ws(3, 8, 12) == 3 * 64 and ws(2, 67, 131) == 2 * 9 * 64 and ws(1, 1080, 1920) == 256 * 64
    assert ws(65535, 2, 2) == 65535 * 64 and ws(1, 32768, 65535) == 256 * 64
    for bad in ((0, 4, 4), (-1, 4, 4), (65536, 4, 4), (1, 1, 4), (1, 4, 1), (1, 0, 0), (1, 65536, 32768), (1, 46341, 46341)):
        assert ws(*bad) == -3, bad
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(4096)      # never dereferenced: every call below is rejected first

    def call(a=one, back=one, sign=-1.0, alpha=0.01, beta=0.5, wsp=one, err=one, cons=one, known=one, rec=one, n=1, h=4, w=4,
             a_bs=0, b_bs=0, a_half=0, b_half=0):
        return lib.ofl_flow_consistency_f32(a, a_bs, a_half, back, b_bs, b_half, null, 0, null, 0, sign, alpha, beta, wsp, err, cons,
                                            known, rec, n, h, w, null)
    for kw in (dict(n=0), dict(n=65536), dict(n=-3), dict(h=1), dict(w=1), dict(h=0, w=0), dict(h=65536, w=32768),
               dict(sign=0.5), dict(sign=0.0), dict(sign=2.0), dict(sign=float('nan')),
               dict(alpha=-1.0), dict(alpha=float('nan')), dict(alpha=float('inf')), dict(beta=-1e-9), dict(beta=float('nan')),
               dict(beta=float('inf')), dict(a=null), dict(back=null), dict(err=null, cons=null, known=null, rec=null),
               dict(wsp=null), dict(a_bs=-1), dict(b_bs=-32), dict(a_half=2), dict(b_half=-1),
               dict(a=ctypes.c_void_p(4098)), dict(back=ctypes.c_void_p(4097), b_half=1), dict(err=ctypes.c_void_p(4098)),
               dict(rec=ctypes.c_void_p(4100)), dict(wsp=ctypes.c_void_p(4100))):
        assert call(**kw) == -3, kw
