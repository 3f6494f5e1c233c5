"""GPU tier of Flow.photometric / photometric_map / photometric_stats (ofl_photometric.hip) against tests/photometric_oracle.py
(DESIGN.md 3.20).  The bars, derived as 3.19's were: the warp is bit-exact against the C oracle and every later step of the map is a single
IEEE operation, so the map is the oracle's BIT FOR BIT; the count and the max are exact; the float64 sum is within count * 2^-52
relative of the exact sum of the oracle's terms (they are not negative, so this bounds ANY summation order); record fields 3 .. 7 are 0;
the loss is the quotient of the call's own record bit for bit; the gradient is within 2^-22 A + ulp32(want) per element, A being the sum
of the absolute contributions, and exactly 0 where the pixel is not known.

Frames (photometric_oracle.FRAMES): 2 x 2, 2 x 5, 5 x 2 (one of whose images has no known pixel), 5 x 7 (less than a wave), 8 x 12,
20 x 28 (3 blocks), 37 x 53 and 67 x 131 (odd, 8 and 35 blocks), 64 x 256 (rows of 4 waves, 64 blocks) and 65 x 257 (one past both),
1 x 1080 x 1920 (the 256 blocks of the image walk 31 or 32 rounds; forward only)."""
import functools

import numpy as np
import pytest
import torch

import photometric_oracle as po

gpu = pytest.mark.gpu
KINDS = ("f32c3", "u8c3", "f32c1", "chw")
EPS = 1e-3
# (ref, kind, masked, half): both refs x every kind of image, then without the mask and with fp16-stored flows
CONFIGS = [(r, k, True, False) for r in po.REFS for k in KINDS] + \
          [(r, k, m, hf) for r in po.REFS for k, m, hf in (("f32c3", False, False), ("f32c3", True, True), ("u8c3", False, True))]
LARGE_CONFIGS = [('s', "f32c3", True, False)]
SMALLER = [f for f in po.FRAMES if f != po.LARGE]


def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _ids(frames):
    return ["%dx%dx%d" % f for f in frames]


@functools.lru_cache(maxsize=None)
def _vecs(n, h, w, ref, half):
    a = po.case(n, h, w, ref)[0]
    a = a.astype(np.float16) if half else a
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _oracle(n, h, w, ref, kind, masked=True, half=False, eps=EPS):
    img, other = po.images(n, h, w, ref, kind)
    return po.compute(_vecs(n, h, w, ref, half), po.case(n, h, w, ref)[1] if masked else None, img, other, ref, eps)


@functools.lru_cache(maxsize=None)
def _grad_oracle(n, h, w, ref, kind, masked=True, half=False, eps=EPS):
    img, other = po.images(n, h, w, ref, kind)
    return po.grad(_vecs(n, h, w, ref, half), po.case(n, h, w, ref)[1] if masked else None, img, other, ref, eps, po.UPSTREAM)


def _flow(n, h, w, ref, half=False, requires_grad=False):
    import oflibpytorch_amd as ofl
    v = torch.from_numpy(_vecs(n, h, w, ref, half).copy()).to(_dev())
    if requires_grad:
        v.requires_grad_(True)
    return ofl.Flow(v, ref, torch.from_numpy(po.case(n, h, w, ref)[1].copy()).to(_dev())), v


def _images(n, h, w, ref, kind):
    return tuple(torch.from_numpy(x.copy()).to(_dev()) for x in po.images(n, h, w, ref, kind))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- bar 1: the map bit for bit, the record, the loss ------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,h,w", po.FRAMES, ids=_ids(po.FRAMES))
def test_map_record_and_loss_against_the_oracle(n, h, w):
    from oflibpytorch_amd import _native, _photometric
    worst = 0.0
    for ref, kind, masked, half in (LARGE_CONFIGS if (n, h, w) == po.LARGE else CONFIGS):
        want = _oracle(n, h, w, ref, kind, masked, half)
        flow, v = _flow(n, h, w, ref, half)
        img, other = _images(n, h, w, ref, kind)
        what = "'%s' %s masked %s half %s" % (ref, kind, masked, half)
        # the binding: map and records of one call
        rec, pmap = _photometric.flow_photometric(v, flow.mask if masked else None, img, other, po.sign_of(ref), EPS, want_map=True)
        assert 'photometric' in _native.last_kernel_name()
        assert pmap.dtype == torch.float32 and pmap.shape == (n, h, w) and rec.dtype == torch.float64 and rec.shape == (n, 8)
        assert np.array_equal(pmap.cpu().numpy().view(np.uint32), want['map'].view(np.uint32)), what      # +0 where not known
        rec = rec.cpu().numpy()
        count, total = want['records'][:, 0], want['records'][:, 1]
        print("%d x %d %s: count %s sum %s (oracle %s) max %s" % (h, w, what, rec[:, 0], rec[:, 1], total, rec[:, 2]))
        assert np.array_equal(rec[:, 0], count) and np.array_equal(rec[:, 2], want['records'][:, 2]), what
        assert not rec[:, 3:].any() and not np.signbit(rec[:, 3:]).any(), what
        err = np.abs(rec[:, 1] - total)
        worst = max(worst, float((err / np.maximum(count * 2.0 ** -52 * total, 1e-300)).max()))
        assert np.all(err <= count * 2.0 ** -52 * total), (what, rec[:, 1], total)
        # the API: the same bits; the loss is the quotient of the call's own record
        kw = dict(eps=EPS, consider_mask=masked)
        assert np.array_equal(flow.photometric_map(img, other, **kw).cpu().numpy().view(np.uint32), want['map'].view(np.uint32)), what
        stats = flow.photometric_stats(img, other, **kw)
        assert stats['count'].dtype == torch.int64 and stats['sum'].dtype == torch.float64
        assert np.array_equal(stats['count'].cpu().numpy(), rec[:, 0].astype(np.int64))
        assert np.array_equal(_bits(stats['sum'].cpu().numpy()), _bits(rec[:, 1])) and np.array_equal(stats['max'].cpu().numpy(), rec[:, 2])
        loss = flow.photometric(img, other, **kw)
        assert 'photometric' in _native.last_kernel_name()
        assert loss.dtype == torch.float32 and loss.shape == (n,) and not loss.requires_grad
        with np.errstate(invalid='ignore', divide='ignore'):
            quotient = (rec[:, 1] / rec[:, 0]).astype(np.float32)
        assert np.array_equal(loss.cpu().numpy().view(np.uint32), quotient.view(np.uint32)), what
        assert np.array_equal(stats['photometric'].cpu().numpy().astype(np.float32).view(np.uint32), quotient.view(np.uint32))
        assert np.array_equal(np.isnan(quotient), count == 0)
    print("%d x %d: map bit for bit; largest sum error %.3f of the bound count * 2^-52" % (h, w, worst))


# ---- bar 2: the gradient --------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,h,w", SMALLER, ids=_ids(SMALLER))
def test_gradient_against_the_float64_oracle(n, h, w):
    from oflibpytorch_amd import _native, _photometric
    worst = 0.0
    up = torch.tensor(po.UPSTREAM[:n], device=_dev())
    for ref, kind, masked, half in CONFIGS:
        for eps in ((EPS, 0.0) if (kind, masked, half) == ("f32c3", True, False) else (EPS,)):
            want, big_a = _grad_oracle(n, h, w, ref, kind, masked, half, eps)
            known = _oracle(n, h, w, ref, kind, masked, half, eps)['known']
            img, other = _images(n, h, w, ref, kind)
            what = "'%s' %s masked %s half %s eps %g" % (ref, kind, masked, half, eps)
            if half:
                # an fp16 leaf takes an fp16 gradient: the kernel's fp32 output is checked through the binding, as autograd calls it
                flow, v = _flow(n, h, w, ref, True)
                mask = flow.mask if masked else None
                rec, _ = _photometric.flow_photometric(v, mask, img, other, po.sign_of(ref), eps)
                scale = (up.double() / rec[:, 0]).float()
                got = _photometric.flow_photometric_grad(v, mask, img, other, po.sign_of(ref), eps, scale)
            else:
                flow, v = _flow(n, h, w, ref, requires_grad=True)
                if img.dtype == torch.float32:
                    img.requires_grad_(True)
                    other.requires_grad_(True)
                loss = flow.photometric(img, other, eps=eps, consider_mask=masked)
                assert loss.requires_grad
                loss.backward(up)
                assert img.grad is None and other.grad is None                                # the images carry no gradient
                got = v.grad
            assert 'flow_photometric_kernel' in _native.last_kernel_name()
            got = got.cpu().numpy()
            assert got.dtype == np.float32 and got.shape == (n, 2, h, w)
            unknown = ~np.broadcast_to(known[:, None], got.shape)
            assert not got[unknown].view(np.uint32).any(), what                               # exactly +0 where not known
            assert np.isfinite(got).all(), what
            assert h * w < 35 or (want != 0).any(), what                                      # the oracle's gradient is not vacuous
            bound = po.grad_bound(want, big_a)
            err = np.abs(got.astype(np.float64) - want)
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (what, float((err / bound).max()))
    print("%d x %d: largest gradient error %.3f of the bound 2^-22 A + ulp32" % (h, w, worst))


# ---- bar 3: an image without a known pixel -------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ref", po.REFS)
def test_an_all_masked_image_is_nan_with_gradient_zero_and_leaves_its_neighbours_alone(ref):
    import oflibpytorch_amd as ofl
    n, h, w = 3, 8, 12
    a, m = po.case(n, h, w, ref)[:2]
    img, other = _images(n, h, w, ref, "f32c3")
    up = torch.tensor(po.UPSTREAM, device=_dev())

    def run(mask):
        v = torch.from_numpy(a.copy()).to(_dev()).requires_grad_(True)
        flow = ofl.Flow(v, ref, torch.from_numpy(mask.copy()).to(_dev()))
        stats = flow.photometric_stats(img, other)
        pmap = flow.photometric_map(img, other)
        loss = flow.photometric(img, other)
        loss.backward(up)
        return [t.cpu().numpy() for t in (stats['count'], stats['sum'], stats['max'], pmap, loss.detach(), v.grad)]
    whole = run(m)
    hole = m.copy()
    hole[1] = False
    holed = run(hole)
    for x, y in zip(whole, holed):
        for i in (0, 2):
            assert np.array_equal(_bits(x[i]), _bits(y[i]))
    count, total, mx, pmap, loss, grad = holed
    assert count[1] == 0 and total[1] == 0 and mx[1] == 0 and not pmap[1].view(np.uint32).any()
    assert np.isnan(loss[1]) and not grad[1].view(np.uint32).any() and np.isfinite(grad).all()
    assert whole[0][1] > 0 and np.abs(whole[5][1]).max() > 0


# ---- bar 4: the anchor on the device -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ref", po.REFS)
@pytest.mark.parametrize("n,h,w", SMALLER[3:], ids=_ids(SMALLER[3:]))
def test_the_map_is_the_warp_of_apply_compared_in_torch(n, h, w, ref):
    """The warped image of Flow.apply on the 't' flow that samples the same positions, its valid area, and the same float32 operations
    in torch: the valid area is the set of known pixels and the map is the same bit for bit."""
    flow, _ = _flow(n, h, w, ref)
    img, other = _images(n, h, w, ref, "f32c3")
    sampler = flow if ref == 't' else flow.invert('t')
    warped, area = sampler.apply(other, return_valid_area=True)
    stats = flow.photometric_stats(img, other, eps=EPS)
    pmap = flow.photometric_map(img, other, eps=EPS)
    assert torch.equal(area, pmap > 0)                                                      # (rho >= eps > 0 where known)
    assert torch.equal(area.sum((1, 2)), stats['count'])
    d = warped - img
    ee = torch.tensor(np.float32(EPS) * np.float32(EPS), device=_dev())
    r = torch.sqrt(d * d + ee)
    # (a division by a tensor: torch turns a division by a Python number into a multiplication by its inverse)
    rho = ((r[:, 0] + r[:, 1]) + r[:, 2]) / torch.tensor(3.0, device=_dev())
    want = torch.where(area, rho, torch.zeros_like(rho))
    assert want.dtype == torch.float32
    assert np.array_equal(pmap.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))


# ---- bar 5: an image's bits do not depend on the batch, its position in it, or the run ----------------------------------------------
@gpu
@pytest.mark.parametrize("ref", po.REFS)
@pytest.mark.parametrize("n,h,w", [(3, 8, 12), (3, 37, 53)], ids=_ids([(3, 8, 12), (3, 37, 53)]))
def test_batch_independence_and_reproducibility(n, h, w, ref):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _photometric
    a, m = (torch.from_numpy(x.copy()).to(_dev()) for x in po.case(n, h, w, ref)[:2])
    img, other = _images(n, h, w, ref, "f32c3")
    up = torch.tensor(po.UPSTREAM, device=_dev())

    def run(idx):
        idx = torch.tensor(idx, device=_dev())
        v = a[idx].clone().requires_grad_(True)
        rec, pmap = _photometric.flow_photometric(v.detach(), m[idx].clone(), img[idx].clone(), other[idx].clone(), po.sign_of(ref), EPS,
                                                  want_map=True)
        loss = ofl.Flow(v, ref, m[idx].clone()).photometric(img[idx].clone(), other[idx].clone(), eps=EPS)
        loss.backward(up[idx])
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (rec, pmap, loss.detach(), v.grad)]
    whole = run([0, 1, 2])
    again = run([0, 1, 2])
    for x, y in zip(whole, again):
        assert np.array_equal(_bits(x), _bits(y))                                           # two runs, gradient included
    moved = run([2, 0, 1])
    for i in range(n):
        alone = run([i])
        for x, y, z in zip(whole, alone, moved):
            j = (i + 1) % 3                                                                 # where image i sits in `moved`
            assert np.array_equal(_bits(x[i:i + 1]), _bits(y[0:1])), i
            assert np.array_equal(_bits(x[i:i + 1]), _bits(z[j:j + 1])), i
