"""GPU tier of Flow.census / census_map / census_stats (ofl_census.hip) against tests/census_oracle.py.  The bars: the
warp is bit-exact against the C oracle and every later step up to b is a single IEEE operation in a fixed order, so with q = 1 (pow(b, 1)
= b) the map is the oracle's BIT FOR BIT; with the default q = 0.4 the float64 pow of two libraries is rounded to float32: within 1
float32 ulp, and exactly +0 where the pixel is not known.  The count, the number of terms and the max are exact; the float64 sum is within
count * 2^-52 relative of the exact sum of the call's own map (its terms are not negative, so this bounds ANY summation order); record
fields 4 .. 7 are 0; the loss is the quotient of the call's own record bit for bit; the gradient is within 2^-22 A + ulp32(want) per
element, A being the sum of the absolute contributions, and exactly 0 where the pixel is not known.

Frames (census_oracle.FRAMES): 2 x 2, 2 x 5, 5 x 2 (narrower than the halo), 5 x 7, 8 x 12, 20 x 28, 37 x 53 and 67 x 131 (odd, 3 x 1
and 5 x 3 tiles), 64 x 256 (4 x 4 whole tiles) and 65 x 257 (one past both), 16 x 64 (exactly the kernel's tile) and 17 x 65 (one past
it: 2 x 2 tiles)."""
import functools
import math

import numpy as np
import pytest
import torch

import census_oracle as cen
import photometric_oracle as po

gpu = pytest.mark.gpu
KINDS = ("f32c3", "u8c3", "f32c1", "chw")
# (ref, kind, masked, half, patch): both refs x every kind of image at patch 7, then without the mask, fp16-stored flows, patches 3 and 5
CONFIGS = [(r, k, True, False, 7) for r in cen.REFS for k in KINDS] + \
          [(r, k, m, hf, p) for r in cen.REFS for k, m, hf, p in (("f32c3", False, False, 7), ("f32c3", True, True, 7), ("u8c3", False, True, 5),
                                                                  ("f32c3", True, False, 3), ("f32c3", True, False, 5),
                                                                  ("u8c3", True, False, 3), ("f32c1", False, True, 3), ("chw", True, False, 5))]
QS = (1.0, cen.Q)
POW_ULPS = 1.0                # q != 1: the float64 pow of two libraries, rounded once to float32


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
def _oracle(n, h, w, ref, kind, masked=True, half=False, patch=7, q=cen.Q):
    img, other = po.images(n, h, w, ref, kind)
    return cen.compute(_vecs(n, h, w, ref, half), po.case(n, h, w, ref)[1] if masked else None, img, other, ref, patch, cen.THRESH,
                       cen.EPS, q)


@functools.lru_cache(maxsize=None)
def _grad_oracle(n, h, w, ref, kind, masked=True, half=False, patch=7, q=cen.Q):
    img, other = po.images(n, h, w, ref, kind)
    return cen.grad(_vecs(n, h, w, ref, half), po.case(n, h, w, ref)[1] if masked else None, img, other, ref, patch, cen.THRESH,
                    cen.EPS, q, cen.UPSTREAM)


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


def _check_record_against_own_map(rec, cmap, what):
    """count, max: those of the call's own map; sum: within count * 2^-52 relative of its exact sum; fields 4 .. 7: +0"""
    worst = 0.0
    for i in range(cmap.shape[0]):
        vals = cmap[i][cmap[i] > 0].astype(np.float64)               # (rho >= eps^q > 0 where known, +0 elsewhere)
        exact = math.fsum(vals.tolist())
        assert rec[i, 0] == vals.size and rec[i, 2] == (vals.max() if vals.size else 0.0), what
        err = abs(rec[i, 1] - exact)
        assert err <= vals.size * 2.0 ** -52 * exact, (what, rec[i, 1], exact)
        worst = max(worst, err / max(vals.size * 2.0 ** -52 * exact, 1e-300))
    assert not rec[:, 4:].any() and not np.signbit(rec[:, 4:]).any(), what
    return worst


# ---- bar 1: the map, the record, the loss ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,h,w", cen.FRAMES, ids=_ids(cen.FRAMES))
def test_map_record_and_loss_against_the_oracle(n, h, w):
    from oflibpytorch_amd import _census, _native
    worst, worst_ulp = 0.0, 0.0
    for ref, kind, masked, half, patch in CONFIGS:
        flow, v = _flow(n, h, w, ref, half)
        img, other = _images(n, h, w, ref, kind)
        for q in QS:
            want = _oracle(n, h, w, ref, kind, masked, half, patch, q)
            what = "'%s' %s masked %s half %s patch %d q %g" % (ref, kind, masked, half, patch, q)
            # the binding: map and records of one call
            rec, cmap = _census.flow_census(v, flow.mask if masked else None, img, other, cen.sign_of(ref), patch, cen.THRESH, cen.EPS, q,
                                            want_map=True)
            assert 'census' in _native.last_kernel_name()
            assert cmap.dtype == torch.float32 and cmap.shape == (n, h, w) and rec.dtype == torch.float64 and rec.shape == (n, 8)
            cmap, rec = cmap.cpu().numpy(), rec.cpu().numpy()
            known = want['known']
            assert not cmap[~known].view(np.uint32).any(), what                                # exactly +0 where not known
            if q == 1.0:
                assert np.array_equal(cmap.view(np.uint32), want['map'].view(np.uint32)), what
            else:
                ulps = np.abs(cmap.astype(np.float64) - want['map']) / cen.ulp32(want['map'])
                worst_ulp = max(worst_ulp, float(ulps[known].max()) if known.any() else 0.0)
                assert np.all(ulps[known] <= POW_ULPS), (what, float(ulps.max()))
                assert np.all(cmap[known] > 0), what
            print("%d x %d %s: count %s terms %s sum %s max %s" % (h, w, what, rec[:, 0], rec[:, 3], rec[:, 1], rec[:, 2]))
            assert np.array_equal(rec[:, 0], want['records'][:, 0]) and np.array_equal(rec[:, 3], want['records'][:, 3]), what
            worst = max(worst, _check_record_against_own_map(rec, cmap, what))
            # the API: the same bits; the loss is the quotient of the call's own record
            kw = dict(patch=patch, q=q, consider_mask=masked)
            assert np.array_equal(flow.census_map(img, other, **kw).cpu().numpy().view(np.uint32), cmap.view(np.uint32)), what
            stats = flow.census_stats(img, other, **kw)
            assert stats['count'].dtype == torch.int64 and stats['sum'].dtype == torch.float64
            assert np.array_equal(stats['count'].cpu().numpy(), rec[:, 0].astype(np.int64))
            assert np.array_equal(_bits(stats['sum'].cpu().numpy()), _bits(rec[:, 1])) and np.array_equal(stats['max'].cpu().numpy(), rec[:, 2])
            with np.errstate(invalid='ignore', divide='ignore'):
                assert np.array_equal(_bits(stats['fill'].cpu().numpy()), _bits(rec[:, 3] / (rec[:, 0] * (patch * patch - 1))))
                quotient = (rec[:, 1] / rec[:, 0]).astype(np.float32)
            loss = flow.census(img, other, **kw)
            assert 'census' in _native.last_kernel_name()
            assert loss.dtype == torch.float32 and loss.shape == (n,) and not loss.requires_grad
            assert np.array_equal(loss.cpu().numpy().view(np.uint32), quotient.view(np.uint32)), what
            assert np.array_equal(stats['census'].cpu().numpy().astype(np.float32).view(np.uint32), quotient.view(np.uint32))
            assert np.array_equal(np.isnan(quotient), rec[:, 0] == 0)
    print("%d x %d: q = 1 bit for bit; q = 0.4 within %.2f ulp; largest sum error %.3f of the bound count * 2^-52" % (h, w, worst_ulp, worst))


# ---- bar 2: the gradient --------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,h,w", cen.FRAMES, ids=_ids(cen.FRAMES))
def test_gradient_against_the_float64_oracle(n, h, w):
    from oflibpytorch_amd import _census, _native
    worst = 0.0
    up = torch.tensor(cen.UPSTREAM[:n], device=_dev())
    for ref, kind, masked, half, patch in CONFIGS:
        for q in (QS if (kind, masked, half, patch) == ("f32c3", True, False, 7) else (cen.Q,)):
            want, big_a = _grad_oracle(n, h, w, ref, kind, masked, half, patch, q)
            known = _oracle(n, h, w, ref, kind, masked, half, patch, q)['known']
            img, other = _images(n, h, w, ref, kind)
            what = "'%s' %s masked %s half %s patch %d q %g" % (ref, kind, masked, half, patch, q)
            if half:
                # an fp16 leaf takes an fp16 gradient: the kernel's fp32 output is checked through the binding, as autograd calls it
                flow, v = _flow(n, h, w, ref, True)
                mask = flow.mask if masked else None
                rec, _ = _census.flow_census(v, mask, img, other, cen.sign_of(ref), patch, cen.THRESH, cen.EPS, q)
                scale = (up.double() / rec[:, 0]).float()
                got = _census.flow_census_grad(v, mask, img, other, cen.sign_of(ref), patch, cen.THRESH, cen.EPS, q, scale)
            else:
                flow, v = _flow(n, h, w, ref, requires_grad=True)
                if img.dtype == torch.float32:
                    img.requires_grad_(True)
                    other.requires_grad_(True)
                loss = flow.census(img, other, patch=patch, q=q, consider_mask=masked)
                assert loss.requires_grad
                loss.backward(up)
                assert img.grad is None and other.grad is None                                # the images carry no gradient
                got = v.grad
            assert 'flow_census_grad_kernel' in _native.last_kernel_name()
            got = got.cpu().numpy()
            assert got.dtype == np.float32 and got.shape == (n, 2, h, w)
            unknown = ~np.broadcast_to(known[:, None], got.shape)
            assert not got[unknown].view(np.uint32).any(), what                               # exactly +0 where not known
            assert np.isfinite(got).all(), what
            assert h * w < 20 * 28 or (want != 0).any((1, 2, 3)).all(), what                  # the oracle's gradient is not vacuous
            bound = cen.grad_bound(want, big_a)
            err = np.abs(got.astype(np.float64) - want)
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (what, float((err / bound).max()))
    print("%d x %d: largest gradient error %.3f of the bound 2^-22 A + ulp32" % (h, w, worst))


# ---- bar 3: the planted case ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ref", cen.REFS)
def test_the_planted_case(ref):
    import oflibpytorch_amd as ofl
    a, mask, img = (torch.from_numpy(x.copy()).to(_dev()) for x in cen.planted())
    v = a.clone().requires_grad_(True)
    flow = ofl.Flow(v, ref, mask)
    cmap = flow.census_map(img, img.clone()).cpu().numpy()[0]
    stats = flow.census_stats(img, img.clone())
    rho = np.float32(np.power(np.float64(np.float32(cen.EPS)), np.float64(np.float32(cen.Q))))
    known = cen.compute(*cen.planted()[:2], cen.planted()[2], cen.planted()[2], ref)['known'][0]
    assert known.sum() == cen.PLANTED_COUNT and not known[cen.PLANTED_LONE] and known[cen.PLANTED_CENTRE]
    assert np.array_equal(cmap[known].view(np.uint32), np.full(cen.PLANTED_COUNT, rho, np.float32).view(np.uint32))
    assert not cmap[~known].view(np.uint32).any() and cmap[cen.PLANTED_LONE] == 0
    assert stats['count'].tolist() == [cen.PLANTED_COUNT] and stats['max'].tolist() == [float(rho)]
    # the terms: the two pixels of the pair have one each; over the pixels of a 7 x 7 block on its own, (rows in reach) x (columns in
    # reach) - 1 adds up to (4 + 5 + 6 + 7 + 6 + 5 + 4)^2 - 49
    assert stats['fill'].tolist() == [(2 + 37 * 37 - 49) / (cen.PLANTED_COUNT * 48.0)]
    flow.census(img, img.clone()).backward(torch.ones(1, device=_dev()))
    grad = v.grad.cpu().numpy()
    assert not grad.any() and not grad[0][:, ~known].view(np.uint32).any()                 # every e is 0: so is every k


# ---- bar 4: an image without a known pixel -------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ref", cen.REFS)
def test_an_all_masked_image_is_nan_with_gradient_zero_and_leaves_its_neighbours_alone(ref):
    import oflibpytorch_amd as ofl
    n, h, w = 3, 8, 12
    a, m = po.case(n, h, w, ref)[:2]
    img, other = _images(n, h, w, ref, "f32c3")
    up = torch.tensor(cen.UPSTREAM, device=_dev())

    def run(mask):
        v = torch.from_numpy(a.copy()).to(_dev()).requires_grad_(True)
        flow = ofl.Flow(v, ref, torch.from_numpy(mask.copy()).to(_dev()))
        stats = flow.census_stats(img, other)
        cmap = flow.census_map(img, other)
        loss = flow.census(img, other)
        loss.backward(up)
        return [t.cpu().numpy() for t in (stats['count'], stats['sum'], stats['max'], cmap, loss.detach(), v.grad)]
    whole = run(m)
    hole = m.copy()
    hole[1] = False
    holed = run(hole)
    for x, y in zip(whole, holed):
        for i in (0, 2):
            assert np.array_equal(_bits(x[i]), _bits(y[i]))
    count, total, mx, cmap, loss, grad = holed
    assert count[1] == 0 and total[1] == 0 and mx[1] == 0 and not cmap[1].view(np.uint32).any()
    assert np.isnan(loss[1]) and not grad[1].view(np.uint32).any() and np.isfinite(grad).all()
    assert whole[0][1] > 0 and np.abs(whole[5][1]).max() > 0


# ---- bar 5: the anchor on the device -----------------------------------------------------------------------------------------------
def _torch_map(warped, area, img, patch, q):
    """The definition in float32 torch operations on the warped image and the valid area of Flow.apply (constants are tensors: torch
    turns an operation with a Python number into another one)"""
    dev = warped.device
    c = {k: torch.tensor(np.float32(x), device=dev) for k, x in (("r", 0.299), ("g", 0.587), ("b", 0.114), ("s", 255.0), ("soft", 0.81),
                                                                 ("th", cen.THRESH), ("eps", cen.EPS))}
    gw = c["s"] * ((c["r"] * warped[:, 0] + c["g"] * warped[:, 1]) + c["b"] * warped[:, 2])
    gi = c["s"] * ((c["r"] * img[:, 0] + c["g"] * img[:, 1]) + c["b"] * img[:, 2])
    n, h, w = area.shape
    r = patch // 2

    def at(x, dy, dx):
        return torch.nn.functional.pad(x, (r, r, r, r))[:, r + dy:r + dy + h, r + dx:r + dx + w]
    total, cnt = torch.zeros_like(gw), torch.zeros_like(gw)
    for dy, dx in cen.offsets(patch):
        term = at(area.float(), dy, dx) > 0
        dw, di = at(gw, dy, dx) - gw, at(gi, dy, dx) - gi
        e = di / torch.sqrt(c["soft"] + di * di) - dw / torch.sqrt(c["soft"] + dw * dw)
        s = e * e
        total = torch.where(term, total + s / (c["th"] + s), total)
        cnt = cnt + term.float()
    known = area & (cnt > 0)
    b = total / cnt + c["eps"]
    rho = torch.pow(b.double(), torch.tensor(np.float64(np.float32(q)), device=dev)).float()
    assert b.dtype == torch.float32
    return torch.where(known, rho, torch.zeros_like(rho)), known


@gpu
@pytest.mark.parametrize("ref", cen.REFS)
@pytest.mark.parametrize("n,h,w", cen.FRAMES[3:], ids=_ids(cen.FRAMES[3:]))
def test_the_map_is_the_warp_of_apply_compared_in_torch(n, h, w, ref):
    """The warped image of Flow.apply on the 't' flow that samples the same positions, its valid area, and the same float32 operations
    in torch: with q = 1 the map is the same bit for bit, with q = 0.4 within 1 float32 ulp."""
    flow, _ = _flow(n, h, w, ref)
    img, other = _images(n, h, w, ref, "f32c3")
    sampler = flow if ref == 't' else flow.invert('t')
    warped, area = sampler.apply(other, return_valid_area=True)
    for patch in cen.PATCHES:
        for q in QS:
            want, known = _torch_map(warped, area, img, patch, q)
            cmap = flow.census_map(img, other, patch=patch, q=q)
            assert torch.equal(known, cmap > 0), (patch, q)
            assert torch.equal(known.sum((1, 2)), flow.census_stats(img, other, patch=patch, q=q)['count'])
            got, want = cmap.cpu().numpy(), want.cpu().numpy()
            if q == 1.0:
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), patch
            else:
                assert np.all(np.abs(got.astype(np.float64) - want) <= cen.ulp32(want)), patch


# ---- bar 6: an image's bits do not depend on the batch, its position in it, or the run ----------------------------------------------
@gpu
@pytest.mark.parametrize("ref", cen.REFS)
@pytest.mark.parametrize("n,h,w", [(3, 8, 12), (3, 37, 53)], ids=_ids([(3, 8, 12), (3, 37, 53)]))
def test_batch_independence_and_reproducibility(n, h, w, ref):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _census
    a, m = (torch.from_numpy(x.copy()).to(_dev()) for x in po.case(n, h, w, ref)[:2])
    img, other = _images(n, h, w, ref, "f32c3")
    up = torch.tensor(cen.UPSTREAM, device=_dev())

    def run(idx):
        idx = torch.tensor(idx, device=_dev())
        v = a[idx].clone().requires_grad_(True)
        rec, cmap = _census.flow_census(v.detach(), m[idx].clone(), img[idx].clone(), other[idx].clone(), cen.sign_of(ref), want_map=True)
        loss = ofl.Flow(v, ref, m[idx].clone()).census(img[idx].clone(), other[idx].clone())
        loss.backward(up[idx])
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (rec, cmap, loss.detach(), v.grad)]
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
