"""GPU tier of the dataset loaders (ofl_loaders.hip): the decode kernels against NumPy bit for bit (vectors, mask,
flag words) over every tail length, aligned and misaligned storage and the edge samples; the public API on the reference's fixtures
(test/test_flow_class.py:205-238: its values and its six error cases); batches; no validation launch; a loaded flow is usable."""
import os
import struct

import numpy as np
import pytest
import torch

import png_oracle as po

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, 'tests', 'golden', 'loaders')
fx = lambda name: os.path.join(FIX, name)

HEIGHTS, WIDTHS = (1, 2, 3), (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65)
EXTRA = [(5, 413)]                                   # 2065 pixels: three blocks of 256 lanes x 4 pixels, a tail of one
KITTI_EDGES = np.array([0, 32767, 32768, 32769, 65535], dtype=np.uint16)
WANT = np.arange(10)[:, None] * np.arange(20)[None, :]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _flow_flags(vecs, mask):
    """The words the constructor's own validation (flow_flags_kernel) forms for these tensors."""
    import oflibpytorch_amd as ofl
    f = ofl.Flow(vecs.clone(), 's') if mask is None else ofl.Flow(vecs.clone(), 's', mask.clone())
    return [int(x) for x in f._flags()]


def _on_device(host: np.ndarray, dev, offset: int):
    """The bytes of `host` ([N, row bytes] uint8) on the device, starting `offset` bytes into a fresh (256-byte aligned) allocation."""
    n, row = host.shape
    store = torch.zeros(n * row + offset + 16, dtype=torch.uint8, device=dev)
    view = store[offset:offset + n * row].view(n, row)
    view.copy_(torch.from_numpy(host))
    assert view.data_ptr() % 256 == offset
    return view


# ---- ofl_decode_kitti ------------------------------------------------------------------------------------------------------
def _kitti_samples(n, h, w, mask_kind, rng):
    s = rng.randint(0, 65536, size=(n, h, w, 3)).astype(np.uint16)
    edge = rng.rand(n, h, w, 3) < 0.5
    s[edge] = KITTI_EDGES[rng.randint(0, 5, size=int(edge.sum()))]
    if mask_kind == 'valid':
        s[..., 2] = np.maximum(s[..., 2], 1)
    elif mask_kind == 'invalid':
        s[..., 2] = 0
    elif mask_kind == 'last':                        # one valid pixel, in the lane that handles the image's tail
        s[..., 2] = 0
        s[:, -1, -1, 2] = 65535
    elif mask_kind == 'zero':                        # a zero flow: every flag bit stays clear
        s[..., :2] = 32768
    return s


def _check_kitti(s, dev, offset, want_mask):
    from oflibpytorch_amd import _native
    n, h, w, _ = s.shape
    raw = _on_device(s.astype('>u2').view(np.uint8).reshape(n, -1), dev, offset)
    vecs, mask, flags = _native.decode_kitti(raw, h, w, want_mask)
    assert 'decode_kitti_kernel' in _native.last_kernel_name()
    want = s[..., :2].astype(np.float64)
    want = np.moveaxis(((want - 2 ** 15) / 64).astype(np.float32), -1, 1)
    assert vecs.dtype == torch.float32 and tuple(vecs.shape) == (n, 2, h, w)
    assert np.array_equal(vecs.cpu().numpy().view(np.int32), np.ascontiguousarray(want).view(np.int32)), (n, h, w, offset)
    if want_mask:
        assert mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), s[..., 2] > 0), (n, h, w, offset)
        assert np.array_equal(mask.view(torch.uint8).cpu().numpy(), (s[..., 2] > 0).astype(np.uint8))     # stored as 0 / 1
    else:
        assert mask is None
    assert flags.cpu().tolist() == _flow_flags(vecs, mask), (n, h, w, offset)
    return flags.cpu().tolist()


@pytest.mark.parametrize("offset", [0, 2], ids=["aligned", "offset2"])
@pytest.mark.parametrize("n", [1, 3])
def test_decode_kitti_bit_for_bit(dev, n, offset):
    rng = np.random.RandomState(100 * n + offset)
    kinds = ('random', 'valid', 'invalid', 'last', 'zero')
    for i, (h, w) in enumerate([(h, w) for h in HEIGHTS for w in WIDTHS] + EXTRA):
        for kind in (kinds if w in (1, 5, 8, 65, 413) else kinds[i % 5:i % 5 + 1]):
            s = _kitti_samples(n, h, w, kind, rng)
            words = _check_kitti(s, dev, offset, True)
            if kind == 'zero':
                assert words == [0] * n
            if kind == 'invalid':
                assert all(wd & 24 == 0 for wd in words)                     # nothing moves under the mask
        _check_kitti(_kitti_samples(n, h, w, 'invalid', rng), dev, offset, False)      # load_valid=False: an all-True mask's flags


def test_decode_kitti_every_storage_offset(dev):
    """Offsets 0 .. 17 bytes: 8-byte aligned ones take the 16 + 8-byte loads (either order), the others the per-sample path."""
    rng = np.random.RandomState(5)
    s = _kitti_samples(2, 3, 23, 'random', rng)
    words = [_check_kitti(s, dev, offset, True) for offset in range(18)]
    assert all(wd == words[0] for wd in words)


# ---- ofl_decode_flo --------------------------------------------------------------------------------------------------------
FLO_EDGES = np.array([-0.0, 0.0, 1e-40, -1e-40, 3.4e38, -3.4e38, 5e-4, -5e-4, 1e-3, -1e-3], dtype=np.float32)


def _flo_values(n, h, w, kind, rng):
    v = (rng.randn(n, h, w, 2) * 3).astype(np.float32)
    edge = rng.rand(n, h, w, 2) < 0.5
    v[edge] = FLO_EDGES[rng.randint(0, len(FLO_EDGES), size=int(edge.sum()))]
    if kind == 'zero':
        v[...] = np.where(rng.rand(n, h, w, 2) < 0.5, np.float32(-0.0), np.float32(0.0))
    elif kind == 'small':                            # non-zero, below the threshold
        v[...] = FLO_EDGES[rng.randint(2, 4, size=v.shape)]      # denormals ...
        v[..., 0] = 5e-4                                          # ... and half the threshold
    return v


def _grey(n, h, w, kind, rng):
    if kind == 'none':
        return None
    g = rng.randint(0, 256, size=(n, h, w)).astype(np.uint8)
    g[rng.rand(n, h, w) < 0.5] = 0
    if kind == 'valid':
        g[...] = 0
    elif kind == 'invalid':
        g[...] = np.maximum(g, 1)
    elif kind == 'last':
        g[...] = 255
        g[:, -1, -1] = 0
    return g


def _check_flo(v, g, dev, offset):
    from oflibpytorch_amd import _native
    n, h, w, _ = v.shape
    raw = _on_device(v.view(np.uint8).reshape(n, -1), dev, offset).view(torch.float32).view(n, h, w, 2)
    grey = None if g is None else torch.from_numpy(g).to(dev)
    vecs, mask, flags = _native.decode_flo(raw, grey)
    assert 'decode_flo_kernel' in _native.last_kernel_name()
    want = np.ascontiguousarray(np.moveaxis(v, -1, 1))
    assert np.array_equal(vecs.cpu().numpy().view(np.int32), want.view(np.int32)), (n, h, w, offset)          # bit patterns
    if g is None:
        assert mask is None
    else:
        assert mask.dtype == torch.bool and np.array_equal(mask.view(torch.uint8).cpu().numpy(), (g == 0).astype(np.uint8))
    words = flags.cpu().tolist()
    if np.isfinite(v).all():
        assert words == _flow_flags(vecs, mask), (n, h, w, offset)
    return words


@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "offset4"])
@pytest.mark.parametrize("n", [1, 3])
def test_decode_flo_bit_for_bit(dev, n, offset):
    rng = np.random.RandomState(200 * n + offset)
    vkinds, gkinds = ('random', 'zero', 'small'), ('none', 'random', 'valid', 'invalid', 'last')
    for i, (h, w) in enumerate([(h, w) for h in HEIGHTS for w in WIDTHS] + EXTRA):
        full = w in (1, 5, 8, 65, 413)
        for vk in (vkinds if full else vkinds[i % 3:i % 3 + 1]):
            for gk in (gkinds if full else gkinds[i % 5:i % 5 + 1]):
                words = _check_flo(_flo_values(n, h, w, vk, rng), _grey(n, h, w, gk, rng), dev, offset)
                if vk == 'zero':
                    assert words == [0] * n
                if vk == 'small':
                    assert all(wd & 2 and not wd & 4 for wd in words)        # non-zero, not beyond the threshold


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_decode_flo_flags_non_finite_values(dev, bad):
    rng = np.random.RandomState(7)
    for (h, w), where in (((3, 7), (2, 6, 1)), ((3, 7), (0, 0, 0)), ((2, 64), (1, 31, 1))):       # the tail lane, the first value, mid-row
        v = _flo_values(2, h, w, 'random', rng)
        v[(1,) + where] = bad
        words = _check_flo(v, _grey(2, h, w, 'random', rng), dev, 0)
        assert words[1] & 1 and not words[0] & 1


def test_grid_stride_and_large_images(dev):
    """More groups than the grid has lanes (2048 blocks x 256 lanes x 4 pixels): the kernels walk on with a grid stride."""
    rng = np.random.RandomState(9)
    h, w = 1, 2048 * 1024 + 4 * 300 + 3
    s = np.full((1, h, w, 3), 32768, dtype=np.uint16)
    s[..., 2] = 0
    s[0, 0, -1] = (32769, 0, 7)                       # the only vector that moves, the only valid pixel: beyond the first sweep
    assert _check_kitti(s, dev, 0, True) == [2 | 4 | 8 | 16]
    s[0, 0, -1, 2] = 0
    assert _check_kitti(s, dev, 8, True) == [2 | 4]
    v = np.zeros((1, h, w, 2), dtype=np.float32)
    v[0, 0, -2] = (0.0, 5e-4)
    g = np.ones((1, h, w), dtype=np.uint8)
    g[0, 0, -2] = 0
    assert _check_flo(v, g, dev, 0) == [2 | 8]
    del rng


# ---- the public API on the reference's fixtures ------------------------------------------------------------------------------
def _expect_device(flow, device):
    want = 'cuda' if (device is not None and torch.device(device).type == 'cuda') else 'cpu'
    assert flow.device.type == want and flow.vecs.device.type == want and flow.mask.device.type == want


@pytest.mark.parametrize("device", [None, 'cpu', 'cuda'])
def test_from_kitti(dev, device):
    import oflibpytorch_amd as ofl
    f = ofl.Flow.from_kitti(fx('kitti.png'), load_valid=True, device=device)
    assert f.shape == (1, 10, 20) and f.ref == 's' and f.vecs.dtype == torch.float32 and f.mask.dtype == torch.bool
    _expect_device(f, device)
    np.testing.assert_equal(f.vecs_numpy[0, ..., 0], WANT)
    np.testing.assert_equal(f.vecs_numpy[0, ..., 1], 0)
    np.testing.assert_equal(f.mask_numpy[0, :, 0], True)
    np.testing.assert_equal(f.mask_numpy[0, :, 10], False)
    g = ofl.Flow.from_kitti(fx('kitti.png'), load_valid=False, device=device)
    _expect_device(g, device)
    np.testing.assert_equal(g.mask_numpy, True)
    assert torch.equal(g.vecs, f.vecs) and ofl.Flow.from_kitti(fx('kitti.png'), device=device).mask.equal(f.mask)      # default: True
    data = ofl.load_kitti(fx('kitti.png'))
    assert data.dtype == torch.float32 and tuple(data.shape) == (3, 10, 20) and data.device.type == 'cpu'
    assert torch.equal(data[:2], f.vecs[0].cpu()) and torch.equal(data[2], f.mask[0].cpu().float())
    with pytest.raises(TypeError, match="Error loading flow from KITTI data: Load_valid needs to be boolean"):
        ofl.Flow.from_kitti(fx('kitti.png'), load_valid='test', device=device)
    with pytest.raises(ValueError, match="Error loading flow from KITTI data: Flow data could not be loaded"):
        ofl.Flow.from_kitti('test', device=device)
    with pytest.raises(ValueError, match="Error loading flow from KITTI data: Loaded flow data has the wrong shape"):
        ofl.Flow.from_kitti(fx('kitti_wrong.png'), device=device)


@pytest.mark.parametrize("device", [None, 'cpu', 'cuda'])
def test_from_sintel(dev, device):
    import oflibpytorch_amd as ofl
    f = ofl.Flow.from_sintel(fx('sintel.flo'), device=device)
    assert f.shape == (1, 10, 20) and f.ref == 's' and f.vecs.dtype == torch.float32 and f.mask.dtype == torch.bool
    _expect_device(f, device)
    np.testing.assert_equal(f.vecs_numpy[0, ..., 0], WANT)
    np.testing.assert_equal(f.mask_numpy, True)
    g = ofl.Flow.from_sintel(fx('sintel.flo'), fx('sintel_invalid.png'), device=device)
    assert g.shape == (1, 10, 20) and g.ref == 's' and g.mask.dtype == torch.bool
    _expect_device(g, device)
    np.testing.assert_equal(g.mask_numpy[0, :, 0], True)
    np.testing.assert_equal(g.mask_numpy[0, :, 10], False)
    assert torch.equal(g.vecs, f.vecs)
    data = ofl.load_sintel(fx('sintel.flo'))
    assert data.dtype == torch.float32 and tuple(data.shape) == (2, 10, 20) and torch.equal(data, f.vecs[0].cpu())
    payload = np.fromfile(fx('sintel.flo'), dtype='<f4', offset=12).reshape(10, 20, 2)
    assert np.array_equal(data.numpy().view(np.int32), np.ascontiguousarray(np.moveaxis(payload, -1, 0)).view(np.int32))
    m = ofl.load_sintel_mask(fx('sintel_invalid.png'))
    assert m.dtype == torch.bool and tuple(m.shape) == (10, 20) and torch.equal(m, g.mask[0].cpu())
    with pytest.raises(ValueError, match="Error loading flow from Sintel data: Path not a valid .flo file"):
        ofl.Flow.from_sintel(fx('sintel_wrong.flo'), device=device)
    with pytest.raises(ValueError, match="Error loading flow from Sintel data: Invalid mask could not be loaded from path"):
        ofl.Flow.from_sintel(fx('sintel.flo'), 'test.png', device=device)
    with pytest.raises(ValueError, match="Error setting flow mask: Input shape does not match the desired shape"):
        ofl.Flow.from_sintel(fx('sintel.flo'), fx('sintel_invalid_wrong.png'), device=device)


def _write_flo(path, v):
    with open(path, 'wb') as f:
        f.write(b'PIEH' + struct.pack('<ii', v.shape[1], v.shape[0]) + v.astype('<f4').tobytes())


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_from_sintel_rejects_non_finite_files(dev, tmp_path, bad):
    """The constructor's own ValueError, and nothing else -- also when the mask is of the wrong size (the vectors' error comes first)."""
    import oflibpytorch_amd as ofl
    v = np.fromfile(fx('sintel.flo'), dtype='<f4', offset=12).reshape(10, 20, 2).copy()
    v[9, 19, 1] = bad
    path = str(tmp_path / 'bad.flo')
    _write_flo(path, v)
    for inv in (None, fx('sintel_invalid.png'), fx('sintel_invalid_wrong.png')):
        with pytest.raises(ValueError, match="Error setting flow vectors: Input contains NaN, Inf or -Inf values"):
            ofl.Flow.from_sintel(path, inv, device='cuda')


def test_batches(dev, tmp_path):
    """A list of paths: one flow, bit for bit the batch of the single loads; frames of different sizes are a ValueError."""
    import oflibpytorch_amd as ofl
    rng = np.random.RandomState(11)
    kitti, flo, inv = [fx('kitti.png')], [fx('sintel.flo')], [fx('sintel_invalid.png')]
    for i in range(2):
        s = _kitti_samples(1, 10, 20, 'random', rng)[0]
        kitti.append(str(tmp_path / ('k%d.png' % i)))
        with open(kitti[-1], 'wb') as f:
            f.write(po.encode(s, 16, 2, filters=[i, 4, 3, 2, 1], idat_split=100))
        flo.append(str(tmp_path / ('s%d.flo' % i)))
        _write_flo(flo[-1], _flo_values(1, 10, 20, 'random', rng)[0])
        inv.append(str(tmp_path / ('m%d.png' % i)))
        with open(inv[-1], 'wb') as f:
            f.write(po.encode((rng.rand(10, 20) < 0.4).astype(np.int64), 1, 0, filters=[2, 1]))
    for load_valid in (True, False):
        batch = ofl.Flow.from_kitti(kitti, load_valid, device='cuda')
        singles = ofl.batch_flows([ofl.Flow.from_kitti(p, load_valid, device='cuda') for p in kitti])
        assert batch.shape == (3, 10, 20) and batch.ref == 's'
        assert torch.equal(batch.vecs.view(torch.int32), singles.vecs.view(torch.int32)) and torch.equal(batch.mask, singles.mask)
        assert batch._flags() == singles._flags()
    assert torch.equal(ofl.load_kitti(tuple(kitti)), torch.stack([ofl.load_kitti(p) for p in kitti]))
    for masks in (None, inv):
        batch = ofl.Flow.from_sintel(flo, masks, device='cuda')
        singles = ofl.batch_flows([ofl.Flow.from_sintel(p, None if masks is None else masks[i], device='cuda') for i, p in enumerate(flo)])
        assert batch.shape == (3, 10, 20)
        assert torch.equal(batch.vecs.view(torch.int32), singles.vecs.view(torch.int32)) and torch.equal(batch.mask, singles.mask)
        assert batch._flags() == singles._flags()
    assert torch.equal(ofl.load_sintel(flo), torch.stack([ofl.load_sintel(p) for p in flo]))
    assert torch.equal(ofl.load_sintel_mask(inv), torch.stack([ofl.load_sintel_mask(p) for p in inv]))
    # mixed sizes
    other = str(tmp_path / 'other.png')
    with open(other, 'wb') as f:
        f.write(po.encode(_kitti_samples(1, 10, 21, 'random', rng)[0], 16, 2))
    with pytest.raises(ValueError, match="equal size"):
        ofl.Flow.from_kitti([kitti[0], other], device='cuda')
    other_flo = str(tmp_path / 'other.flo')
    _write_flo(other_flo, _flo_values(1, 12, 20, 'random', rng)[0])
    with pytest.raises(ValueError, match="equal size"):
        ofl.Flow.from_sintel([flo[0], other_flo], device='cuda')
    with pytest.raises(ValueError, match="equal numbers"):
        ofl.Flow.from_sintel(flo, inv[:2], device='cuda')
    with pytest.raises(ValueError, match="Error setting flow mask: Input shape does not match the desired shape"):
        ofl.Flow.from_sintel(flo, [inv[0], fx('sintel_invalid_wrong.png'), inv[2]], device='cuda')


def test_loading_launches_no_validation_kernel(dev):
    """The flag words come out of the decode kernel: building the flow, and then asking what the constructor's validation would have
    asked, launches nothing after it."""
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _native
    for load, name in ((lambda: ofl.Flow.from_kitti(fx('kitti.png'), device='cuda'), 'decode_kitti_kernel'),
                       (lambda: ofl.Flow.from_kitti(fx('kitti.png'), False, device='cuda'), 'decode_kitti_kernel'),
                       (lambda: ofl.Flow.from_sintel(fx('sintel.flo'), device='cuda'), 'decode_flo_kernel'),
                       (lambda: ofl.Flow.from_sintel(fx('sintel.flo'), fx('sintel_invalid.png'), device='cuda'), 'decode_flo_kernel')):
        ofl.Flow(torch.ones(1, 2, 4, 4, device=dev), 's')                    # (the recorder now names the validation kernel)
        assert 'flow_flags' in _native.last_kernel_name()
        f = load()
        assert name in _native.last_kernel_name()
        words = f._flags()
        zero = f.is_zero(thresholded=True)
        assert name in _native.last_kernel_name() and f._flags_known()
        assert words == _flow_flags(f.vecs, f.mask) and not bool(zero)


def test_loaded_flow_is_usable(dev):
    import oflibpytorch_amd as ofl
    f = ofl.Flow.from_sintel(fx('sintel.flo'), fx('sintel_invalid.png'), device='cuda')
    g = ofl.Flow(f.vecs.clone(), 's', f.mask.clone())
    a, b = f.switch_ref(), g.switch_ref()
    assert a.ref == b.ref == 't'
    assert torch.equal(a.vecs.view(torch.int32), b.vecs.view(torch.int32)) and torch.equal(a.mask, b.mask)
    k = ofl.Flow.from_kitti(fx('kitti.png'), device='cuda')
    a, b = k.switch_ref(), ofl.Flow(k.vecs.clone(), 's', k.mask.clone()).switch_ref()
    assert torch.equal(a.vecs.view(torch.int32), b.vecs.view(torch.int32)) and torch.equal(a.mask, b.mask)
