"""GPU tier of Flow.visualise / visualise_flow (ofl_visualise.hip): bit-exact against the reference's output
(tests/golden/vis.npz) and against the oracle (tests/vis_oracle.py) over modes, masks, borders and ranges, at small sizes and
at 1080p; fp16-stored flows; degenerate flows and masks; batch and run-to-run identity."""
import numpy as np
import pytest
import torch

import vis_cases
import vis_oracle as vo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _smooth(n, h, w, scale, seed, dev):
    g = torch.Generator().manual_seed(seed)
    lo = torch.randn(n, 2, 5, 7, generator=g) * scale
    f = torch.nn.functional.interpolate(lo, size=(h, w), mode='bicubic', align_corners=True)
    f[:, :, : h // 7, : w // 9] = 0                         # a patch of zero vectors (zero magnitude)
    return f.contiguous().to(dev)


def _mask(n, h, w, seed, dev):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(n, h, w, generator=g) > 0.2
    m[:, h // 4: h // 2, w // 3: w // 2] = False
    return m.to(dev)


def _oracle_all(flow, mask, show_mask, borders, rng):
    """{mode: N-H-W-3} from one set of oracle HSV planes"""
    hsv = vo.hsv_planes(flow.cpu().float().numpy(), None if mask is None else mask.cpu().numpy(), show_mask, borders, rng)
    rgb = vo.hsv_to_rgb(hsv)
    return {'hsv': np.round(hsv).astype(np.uint8), 'rgb': rgb, 'bgr': rgb[..., ::-1]}


def _check_all_modes(fl, flow, mask, show_mask, borders, rm):
    n = flow.shape[0]
    rng = None if rm is None else np.broadcast_to(np.asarray(rm, np.float64), (n,))
    exp = _oracle_all(flow, mask, show_mask, borders, rng)
    for mode in ('hsv', 'rgb', 'bgr'):
        got = fl.visualise(mode, show_mask, borders, rm, return_tensor=False)
        assert isinstance(got, np.ndarray) and np.array_equal(got, exp[mode]), (mode, show_mask, borders, rm)
    t = fl.visualise('bgr', show_mask, borders, rm)
    assert isinstance(t, torch.Tensor) and t.device == flow.device and t.dtype == torch.uint8
    assert np.array_equal(t.cpu().numpy(), np.moveaxis(exp['bgr'], -1, 1))


@pytest.mark.parametrize("k", vis_cases.case_ids())
def test_reference_fixture_on_gpu(k, dev):
    import oflibpytorch_amd as ofl
    meta, flow, mask, expected = vis_cases.case(k)
    out, err = vis_cases.run_api(ofl, meta, flow, mask, dev)
    if meta['error'] is not None:
        assert err is not None and list(err) == meta['error']
        return
    assert err is None, err
    if meta['returned'] == 'tensor':
        assert isinstance(out, torch.Tensor) and out.device == (dev if meta['tensor'] else torch.device('cpu'))
        out = out.cpu().numpy()
    else:
        assert isinstance(out, np.ndarray)
    assert out.dtype == np.uint8 and out.shape == expected.shape
    assert np.array_equal(out, expected)


@pytest.mark.parametrize("shape", [(3, 37, 53), (2, 40, 64), (1, 1, 1), (2, 1, 3), (1, 3, 1), (2, 2, 2), (1, 5, 7)])
@pytest.mark.parametrize("rm", [None, 3.5, 'list'])
def test_modes_masks_ranges_against_oracle(shape, rm, dev):
    import oflibpytorch_amd as ofl
    n, h, w = shape
    flow = _smooth(n, h, w, 5.0, 3 + h, dev)
    mask = _mask(n, h, w, 4 + w, dev)
    mask[:, 0, 0] = True                                     # (every image keeps a valid pixel)
    rm = [0.5 + i for i in range(n)] if rm == 'list' else rm
    fl = ofl.Flow(flow, 't', mask)
    for show_mask in (False, True):
        for borders in (False, True):
            _check_all_modes(fl, flow, mask, show_mask, borders, rm)


def test_full_hd_batch_of_four(dev):
    import oflibpytorch_amd as ofl
    n, h, w = 4, 1080, 1920
    flow = _smooth(n, h, w, 12.0, 21, dev)
    mask = _mask(n, h, w, 22, dev)
    fl = ofl.Flow(flow, 't', mask)
    for show_mask, borders, rm in ((False, False, None), (True, True, None), (False, False, [1.0, 2.0, 40.0, 7.5])):
        rng = None if rm is None else np.asarray(rm, np.float64)
        exp = _oracle_all(flow, mask, show_mask, borders, rng)
        assert np.array_equal(fl.visualise('bgr', show_mask, borders, rm).cpu().numpy(), np.moveaxis(exp['bgr'], -1, 1))
        assert np.array_equal(fl.visualise('hsv', show_mask, borders, rm), exp['hsv'])
    # the device range against np.percentile over 2 million values per image
    from oflibpytorch_amd import _native
    v = flow.cpu().numpy()
    mag, _ = vo.cart_to_polar(vo.threshold(v[:, 0]), vo.threshold(v[:, 1]))
    for m in (None, mask):
        rng, counts = _native.visualise_range(flow, m)
        exp = vo.default_range(mag, None if m is None else m.cpu().numpy())
        assert np.array_equal(rng.cpu().numpy(), exp)


def test_fp16_stored_flow(dev):
    import oflibpytorch_amd as ofl
    for (n, h, w) in ((2, 37, 53), (3, 48, 64)):
        f16 = _smooth(n, h, w, 6.0, 31 + w, dev).half()
        mask = _mask(n, h, w, 32, dev)
        fl = ofl.Flow(f16, 't', mask)
        assert fl._half is not None                           # (read as fp16 planes by the kernels)
        for show_mask, borders, rm in ((False, False, None), (True, True, None), (True, False, 2.0)):
            rng = None if rm is None else np.full(n, rm, np.float64)
            exp = _oracle_all(f16.float(), mask, show_mask, borders, rng)
            assert np.array_equal(fl.visualise('rgb', show_mask, borders, rm).cpu().numpy(), np.moveaxis(exp['rgb'], -1, 1))
            assert np.array_equal(fl.visualise('hsv', show_mask, borders, rm), exp['hsv'])
        assert fl._half is not None


def test_constant_and_zero_flows(dev):
    import oflibpytorch_amd as ofl
    n, h, w = 2, 270, 480
    const = torch.zeros(n, 2, h, w, device=dev)
    const[:, 0], const[:, 1] = 3.0, -4.0                    # every pixel in one histogram bin
    for flow in (const, torch.zeros(n, 2, h, w, device=dev), torch.full((n, 2, h, w), 5e-4, device=dev)):
        fl = ofl.Flow(flow, 't')
        _check_all_modes(fl, flow, None, False, False, None)
        _check_all_modes(fl, flow, None, True, True, None)


def test_masks_with_few_valid_pixels(dev):
    import oflibpytorch_amd as ofl
    n, h, w = 3, 30, 41
    flow = _smooth(n, h, w, 4.0, 41, dev)
    mask = torch.zeros(n, h, w, dtype=torch.bool, device=dev)
    mask[1, 7, 9] = True
    mask[2, 0, 0] = mask[2, 29, 40] = True
    fl = ofl.Flow(flow[1:], 't', mask[1:])
    for borders in (False, True):
        _check_all_modes(fl, flow[1:], mask[1:], True, borders, None)
    with pytest.raises(IndexError, match="index -1 is out of bounds for axis 0 with size 0"):
        ofl.Flow(flow, 't', mask).visualise('bgr', show_mask=True)
    _check_all_modes(ofl.Flow(flow, 't', mask), flow, mask, False, True, None)      # (no show_mask: all pixels count)


def test_batch_equals_single_images_and_is_reproducible(dev):
    import oflibpytorch_amd as ofl
    n, h, w = 64, 45, 70
    flow = _smooth(n, h, w, 8.0, 51, dev) * torch.linspace(0.1, 3, n, device=dev).view(n, 1, 1, 1)
    mask = _mask(n, h, w, 52, dev)
    fl = ofl.Flow(flow, 't', mask)
    for args in (('bgr', False, False), ('rgb', True, True)):
        a = fl.visualise(*args)
        b = fl.visualise(*args)
        assert torch.equal(a, b)
        singles = torch.cat([ofl.Flow(flow[i:i + 1], 't', mask[i:i + 1]).visualise(*args) for i in range(n)])
        assert torch.equal(a, singles)


def test_visualise_flow_on_device(dev):
    import oflibpytorch_amd as ofl
    flow = _smooth(1, 33, 47, 3.0, 61, dev)
    exp = _oracle_all(flow, None, False, False, None)
    out = ofl.visualise_flow(flow[0], 'bgr')
    assert out.shape == (3, 33, 47) and out.device == dev
    assert np.array_equal(out.cpu().numpy(), np.moveaxis(exp['bgr'][0], -1, 0))
    assert np.array_equal(ofl.visualise_flow(flow, 'hsv'), exp['hsv'])
