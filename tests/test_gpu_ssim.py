"""GPU tier of Flow.ssim / ssim_map / ssim_stats (ofl_ssim.hip) against tests/ssim_oracle.py.  The bars: the warp is
bit-exact against the C oracle and every later step is a single IEEE operation in a fixed order, so the map is the oracle's BIT FOR BIT,
and exactly +0 where the pixel is not known.  The count, the number of window pixels and the max are exact; the float64 sum is within
count * 2^-52 relative of the exact sum of the call's own map (its terms are not negative, so this bounds ANY summation order); record
fields 4 .. 7 are 0; the loss is the quotient of the call's own record bit for bit; the gradient is within 2^-22 A + ulp32(want) per
element, A being the sum of the absolute contributions, and exactly 0 where the pixel is not known.

Frames (ssim_oracle.FRAMES): 2 x 2, 2 x 5, 5 x 2 (narrower than the halo), 5 x 7, 8 x 12, 20 x 28, 37 x 53 and 67 x 131 (odd, 3 x 1
and 5 x 3 tiles), 64 x 256 (4 x 4 whole tiles) and 65 x 257 (one past both), 16 x 64 (exactly the kernel's tile) and 17 x 65 (one past
it: 2 x 2 tiles)."""
import functools
import math

import numpy as np
import pytest
import torch

import photometric_oracle as po
import ssim_oracle as so

gpu = pytest.mark.gpu
KINDS = ("f32c3", "u8c3", "f32c1", "chw")
# (ref, kind, masked, half, window): both refs x every kind of image at window 3, then without the mask, fp16-stored flows, windows 5
# and 7
CONFIGS = [(r, k, True, False, 3) for r in so.REFS for k in KINDS] + \
          [(r, k, m, hf, win) for r in so.REFS for k, m, hf, win in (("f32c3", False, False, 3), ("f32c3", True, True, 3), ("u8c3", False, True, 5),
                                                                     ("f32c3", True, False, 7), ("f32c3", True, False, 5),
                                                                     ("u8c3", True, False, 7), ("f32c1", False, True, 7), ("chw", True, False, 5))]


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
def _oracle(n, h, w, ref, kind, masked=True, half=False, window=3):
    img, other = po.images(n, h, w, ref, kind)
    return so.compute(_vecs(n, h, w, ref, half), po.case(n, h, w, ref)[1] if masked else None, img, other, ref, window)


def _grad_oracle(n, h, w, ref, kind, masked=True, half=False, window=3):
    img, other = po.images(n, h, w, ref, kind)
    return so.grad(_vecs(n, h, w, ref, half), po.case(n, h, w, ref)[1] if masked else None, img, other, ref, window, so.C1, so.C2,
                   so.UPSTREAM, res=_oracle(n, h, w, ref, kind, masked, half, window))


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


def check_record_against_own_map(rec, smap, known, what):
    """count, max: those of the call's own map over the known pixels; sum: within count * 2^-52 relative of its exact sum; fields
    4 .. 7: +0"""
    worst = 0.0
    for i in range(smap.shape[0]):
        vals = smap[i][known[i]].astype(np.float64)
        exact = math.fsum(vals.tolist())
        assert rec[i, 0] == vals.size and rec[i, 2] == (vals.max() if vals.size else 0.0), what
        err = abs(rec[i, 1] - exact)
        assert err <= vals.size * 2.0 ** -52 * exact, (what, rec[i, 1], exact)
        worst = max(worst, err / max(vals.size * 2.0 ** -52 * exact, 1e-300))
    assert not rec[:, 4:].any() and not np.signbit(rec[:, 4:]).any(), what
    return worst


# ---- bar 1: the map, the record, the loss ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,h,w", so.FRAMES, ids=_ids(so.FRAMES))
def test_map_record_and_loss_against_the_oracle(n, h, w):
    from oflibpytorch_amd import _native, _ssim
    worst = 0.0
    for ref, kind, masked, half, window in CONFIGS:
        flow, v = _flow(n, h, w, ref, half)
        img, other = _images(n, h, w, ref, kind)
        want = _oracle(n, h, w, ref, kind, masked, half, window)
        what = "'%s' %s masked %s half %s window %d" % (ref, kind, masked, half, window)
        # the binding: map and records of one call
        rec, smap = _ssim.flow_ssim(v, flow.mask if masked else None, img, other, so.sign_of(ref), window, so.C1, so.C2, want_map=True)
        assert 'flow_ssim_finish_kernel' in _native.last_kernel_name()
        assert smap.dtype == torch.float32 and smap.shape == (n, h, w) and rec.dtype == torch.float64 and rec.shape == (n, 8)
        smap, rec = smap.cpu().numpy(), rec.cpu().numpy()
        known = want['known']
        assert not smap[~known].view(np.uint32).any(), what                                    # exactly +0 where not known
        assert np.array_equal(smap.view(np.uint32), want['map'].view(np.uint32)), what         # bit for bit
        print("%d x %d %s: count %s window pixels %s sum %s max %s" % (h, w, what, rec[:, 0], rec[:, 3], rec[:, 1], rec[:, 2]))
        assert np.array_equal(rec[:, 0], want['records'][:, 0]) and np.array_equal(rec[:, 3], want['records'][:, 3]), what
        assert np.array_equal(rec[:, 2], want['records'][:, 2]), what
        worst = max(worst, check_record_against_own_map(rec, smap, known, what))
        # the API: the same bits; the loss is the quotient of the call's own record
        kw = dict(window=window, consider_mask=masked)
        assert np.array_equal(flow.ssim_map(img, other, **kw).cpu().numpy().view(np.uint32), smap.view(np.uint32)), what
        assert 'flow_ssim_kernel' in _native.last_kernel_name()
        stats = flow.ssim_stats(img, other, **kw)
        assert stats['count'].dtype == torch.int64 and stats['sum'].dtype == torch.float64
        assert np.array_equal(stats['count'].cpu().numpy(), rec[:, 0].astype(np.int64))
        assert np.array_equal(_bits(stats['sum'].cpu().numpy()), _bits(rec[:, 1])) and np.array_equal(stats['max'].cpu().numpy(), rec[:, 2])
        with np.errstate(invalid='ignore', divide='ignore'):
            assert np.array_equal(_bits(stats['fill'].cpu().numpy()), _bits(rec[:, 3] / (rec[:, 0] * (window * window))))
            quotient = (rec[:, 1] / rec[:, 0]).astype(np.float32)
        loss = flow.ssim(img, other, **kw)
        assert 'ssim' in _native.last_kernel_name()
        assert loss.dtype == torch.float32 and loss.shape == (n,) and not loss.requires_grad
        assert np.array_equal(loss.cpu().numpy().view(np.uint32), quotient.view(np.uint32)), what
        assert np.array_equal(stats['ssim'].cpu().numpy().astype(np.float32).view(np.uint32), quotient.view(np.uint32))
        assert np.array_equal(np.isnan(quotient), rec[:, 0] == 0)
    print("%d x %d: the map bit for bit; largest sum error %.3f of the bound count * 2^-52" % (h, w, worst))


# ---- bar 2: the gradient --------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,h,w", so.FRAMES, ids=_ids(so.FRAMES))
def test_gradient_against_the_float64_oracle(n, h, w):
    from oflibpytorch_amd import _native, _ssim
    worst = 0.0
    up = torch.tensor(so.UPSTREAM[:n], device=_dev())
    for ref, kind, masked, half, window in CONFIGS:
        want, big_a = _grad_oracle(n, h, w, ref, kind, masked, half, window)
        known = _oracle(n, h, w, ref, kind, masked, half, window)['known']
        img, other = _images(n, h, w, ref, kind)
        what = "'%s' %s masked %s half %s window %d" % (ref, kind, masked, half, window)
        if half:
            # an fp16 leaf takes an fp16 gradient: the kernel's fp32 output is checked through the binding, as autograd calls it
            flow, v = _flow(n, h, w, ref, True)
            mask = flow.mask if masked else None
            rec, _ = _ssim.flow_ssim(v, mask, img, other, so.sign_of(ref), window, so.C1, so.C2)
            scale = (up.double() / rec[:, 0]).float()
            got = _ssim.flow_ssim_grad(v, mask, img, other, so.sign_of(ref), window, so.C1, so.C2, scale)
        else:
            flow, v = _flow(n, h, w, ref, requires_grad=True)
            if img.dtype == torch.float32:
                img.requires_grad_(True)
                other.requires_grad_(True)
            loss = flow.ssim(img, other, window=window, consider_mask=masked)
            assert loss.requires_grad
            loss.backward(up)
            assert img.grad is None and other.grad is None                                # the images carry no gradient
            got = v.grad
        assert 'flow_ssim_grad_kernel' in _native.last_kernel_name()
        got = got.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (n, 2, h, w)
        unknown = ~np.broadcast_to(known[:, None], got.shape)
        assert not got[unknown].view(np.uint32).any(), what                               # exactly +0 where not known
        assert np.isfinite(got).all(), what
        assert h * w < 20 * 28 or (want != 0).any((1, 2, 3)).all(), what                  # the oracle's gradient is not vacuous
        bound = so.grad_bound(want, big_a)
        err = np.abs(got.astype(np.float64) - want)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (what, float((err / bound).max()))
    print("%d x %d: largest gradient error %.3f of the bound 2^-22 A + ulp32" % (h, w, worst))


# ---- bar 3: the planted cases ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("window", so.WINDOWS)
@pytest.mark.parametrize("ref", so.REFS)
def test_identical_images_give_exactly_zero(ref, window):
    import oflibpytorch_amd as ofl
    import census_oracle as cen
    a, mask, img = (torch.from_numpy(x.copy()).to(_dev()) for x in so.planted_identical())
    v = a.clone().requires_grad_(True)
    flow = ofl.Flow(v, ref, mask)
    smap = flow.ssim_map(img, img.clone(), window=window).cpu().numpy()[0]
    stats = flow.ssim_stats(img, img.clone(), window=window)
    host = so.planted_identical()
    want = so.compute(host[0], host[1], host[2], host[2], ref, window)
    known = want['known'][0]
    assert known.sum() == so.PLANTED_IDENTICAL_COUNT and known[cen.PLANTED_LONE] and all(known[p] for p in cen.PLANTED_PAIR)
    assert not smap.view(np.uint32).any()                                                  # +0 on every pixel, the known ones included
    assert stats['count'].tolist() == [so.PLANTED_IDENTICAL_COUNT] and stats['max'].tolist() == [0.0] and stats['sum'].tolist() == [0.0]
    assert stats['fill'].tolist() == [want['records'][0, 3] / (so.PLANTED_IDENTICAL_COUNT * float(window * window))]
    flow.ssim(img, img.clone(), window=window).backward(torch.ones(1, device=_dev()))
    grad = v.grad.cpu().numpy()
    want_g, big_a = so.grad(host[0], host[1], host[2], host[2], ref, window, upstream=(1.0,))
    assert np.all(np.abs(grad.astype(np.float64) - want_g) <= so.grad_bound(want_g, big_a))
    assert np.all(np.abs(grad) <= so.grad_bound(np.zeros_like(want_g), big_a))             # within its bound of 0
    assert not grad[0][:, ~known].view(np.uint32).any()


@gpu
@pytest.mark.parametrize("window", so.WINDOWS)
def test_the_clamp_case_bit_for_bit(window):
    import oflibpytorch_amd as ofl
    a, img, other = so.planted_clamp()
    want = so.compute(a, None, img, other, 's', window)
    assert (want['raw'] < 0).sum() >= 50
    flow = ofl.Flow(torch.from_numpy(a.copy()).to(_dev()), 's')
    got = flow.ssim_map(torch.from_numpy(img.copy()).to(_dev()), torch.from_numpy(other.copy()).to(_dev()), window=window).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want['map'].view(np.uint32))
    assert not np.signbit(got).any() and (got == 0).any()


# ---- bar 4: an image without a known pixel -------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ref", so.REFS)
def test_an_all_masked_image_is_nan_with_gradient_zero_and_leaves_its_neighbours_alone(ref):
    import oflibpytorch_amd as ofl
    n, h, w = 3, 8, 12
    a, m = po.case(n, h, w, ref)[:2]
    img, other = _images(n, h, w, ref, "f32c3")
    up = torch.tensor(so.UPSTREAM, device=_dev())

    def run(mask):
        v = torch.from_numpy(a.copy()).to(_dev()).requires_grad_(True)
        flow = ofl.Flow(v, ref, torch.from_numpy(mask.copy()).to(_dev()))
        stats = flow.ssim_stats(img, other)
        smap = flow.ssim_map(img, other)
        loss = flow.ssim(img, other)
        loss.backward(up)
        return [t.cpu().numpy() for t in (stats['count'], stats['sum'], stats['max'], smap, loss.detach(), v.grad)]
    whole = run(m)
    hole = m.copy()
    hole[1] = False
    holed = run(hole)
    for x, y in zip(whole, holed):
        for i in (0, 2):
            assert np.array_equal(_bits(x[i]), _bits(y[i]))
    count, total, mx, smap, loss, grad = holed
    assert count[1] == 0 and total[1] == 0 and mx[1] == 0 and not smap[1].view(np.uint32).any()
    assert np.isnan(loss[1]) and not grad[1].view(np.uint32).any() and np.isfinite(grad).all()
    assert whole[0][1] > 0 and np.abs(whole[5][1]).max() > 0


# ---- bar 5: the anchor on the device -----------------------------------------------------------------------------------------------
def _torch_map(warped, area, img, window):
    """The definition in float32 torch operations on the warped image and the valid area of Flow.apply, on shifted slices in the
    definition's order (constants are tensors: torch turns an operation with a Python number into another one)"""
    dev = warped.device
    c = {k: torch.tensor(np.float32(x), device=dev) for k, x in (("c1", so.C1), ("c2", so.C2), ("one", 1.0), ("two", 2.0), ("half", 0.5),
                                                                 ("zero", 0.0), ("chan", float(warped.shape[1])))}
    n, h, w = area.shape
    r = window // 2

    def at(x, dy, dx):
        return torch.nn.functional.pad(x, (r, r, r, r))[:, r + dy:r + dy + h, r + dx:r + dx + w]
    terms = [at(area.float(), dy, dx) > 0 for dy, dx in so.offsets(window)]
    cnt = torch.zeros((n, h, w), device=dev)
    for term in terms:
        cnt = cnt + term.float()
    total = None
    for ch in range(warped.shape[1]):
        x, y = warped[:, ch], img[:, ch]
        xs, ys = [at(x, dy, dx) for dy, dx in so.offsets(window)], [at(y, dy, dx) for dy, dx in so.offsets(window)]
        sx, sy = torch.zeros_like(x), torch.zeros_like(x)
        for term, xo, yo in zip(terms, xs, ys):
            sx, sy = torch.where(term, sx + xo, sx), torch.where(term, sy + yo, sy)
        mux, muy = sx / cnt, sy / cnt
        vxx, vyy, vxy = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
        for term, xo, yo in zip(terms, xs, ys):
            ax, ay = xo - mux, yo - muy
            vxx, vyy, vxy = torch.where(term, vxx + ax * ax, vxx), torch.where(term, vyy + ay * ay, vyy), torch.where(term, vxy + ax * ay, vxy)
        l1 = (c["two"] * mux) * muy + c["c1"]
        l2 = (mux * mux + muy * muy) + c["c1"]
        s1 = c["two"] * (vxy / cnt) + c["c2"]
        s2 = (vxx / cnt + vyy / cnt) + c["c2"]
        d = (c["one"] - (l1 * s1) / (l2 * s2)) * c["half"]
        d = torch.where(d < 0, c["zero"], torch.where(d > 1, c["one"], d))
        total = d if total is None else total + d
    rho = total / c["chan"]
    assert rho.dtype == torch.float32
    return torch.where(area, rho, torch.zeros_like(rho))


@gpu
@pytest.mark.parametrize("ref", so.REFS)
@pytest.mark.parametrize("n,h,w", so.FRAMES[3:], ids=_ids(so.FRAMES[3:]))
def test_the_map_is_the_warp_of_apply_compared_in_torch(n, h, w, ref):
    """The warped image of Flow.apply on the 't' flow that samples the same positions, its valid area, and the same float32 operations
    in torch: the map is the same bit for bit at every window."""
    flow, _ = _flow(n, h, w, ref)
    img, other = _images(n, h, w, ref, "f32c3")
    sampler = flow if ref == 't' else flow.invert('t')
    warped, area = sampler.apply(other, return_valid_area=True)
    for window in so.WINDOWS:
        want = _torch_map(warped, area, img, window)
        smap = flow.ssim_map(img, other, window=window)
        assert torch.equal(area.sum((1, 2)), flow.ssim_stats(img, other, window=window)['count'])
        assert not smap[~area].cpu().numpy().view(np.uint32).any(), window
        assert np.array_equal(smap.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32)), window


# ---- bar 6: an image's bits do not depend on the batch, its position in it, or the run ----------------------------------------------
@gpu
@pytest.mark.parametrize("ref", so.REFS)
@pytest.mark.parametrize("n,h,w", [(3, 8, 12), (3, 37, 53)], ids=_ids([(3, 8, 12), (3, 37, 53)]))
def test_batch_independence_and_reproducibility(n, h, w, ref):
    import oflibpytorch_amd as ofl
    from oflibpytorch_amd import _ssim
    a, m = (torch.from_numpy(x.copy()).to(_dev()) for x in po.case(n, h, w, ref)[:2])
    img, other = _images(n, h, w, ref, "f32c3")
    up = torch.tensor(so.UPSTREAM, device=_dev())

    def run(idx, window):
        idx = torch.tensor(idx, device=_dev())
        v = a[idx].clone().requires_grad_(True)
        rec, smap = _ssim.flow_ssim(v.detach(), m[idx].clone(), img[idx].clone(), other[idx].clone(), so.sign_of(ref), window, want_map=True)
        loss = ofl.Flow(v, ref, m[idx].clone()).ssim(img[idx].clone(), other[idx].clone(), window=window)
        loss.backward(up[idx])
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (rec, smap, loss.detach(), v.grad)]
    for window in (3, 7):
        whole = run([0, 1, 2], window)
        again = run([0, 1, 2], window)
        for x, y in zip(whole, again):
            assert np.array_equal(_bits(x), _bits(y))                                       # two runs, gradient included
        moved = run([2, 0, 1], window)
        for i in range(n):
            alone = run([i], window)
            for x, y, z in zip(whole, alone, moved):
                j = (i + 1) % 3                                                             # where image i sits in `moved`
                assert np.array_equal(_bits(x[i:i + 1]), _bits(y[0:1])), i
                assert np.array_equal(_bits(x[i:i + 1]), _bits(z[j:j + 1])), i


# ---- bar 7: a NaN in img reaches the windows that hold it, and nothing else ---------------------------------------------------------
@gpu
@pytest.mark.parametrize("window", so.WINDOWS)
@pytest.mark.parametrize("ref", so.REFS)
def test_one_nan_in_img_reaches_exactly_the_windows_that_hold_it(ref, window):
    import oflibpytorch_amd as ofl
    n, h, w = 2, 20, 28
    a, m, img, other, _, _ = po.case(n, h, w, ref)
    clean = _oracle(n, h, w, ref, "f32c3", True, False, window)
    known = clean['known']
    ys, xs = np.nonzero(known[1])
    at = (int(ys[len(ys) // 2]), int(xs[len(ys) // 2]))                                     # a usable pixel of image 1
    dirty = img.copy()
    dirty[1, 1, at[0], at[1]] = np.nan
    flow = ofl.Flow(torch.from_numpy(a.copy()).to(_dev()), ref, torch.from_numpy(m.copy()).to(_dev()))
    other_d = torch.from_numpy(other.copy()).to(_dev())
    got = flow.ssim_map(torch.from_numpy(dirty).to(_dev()), other_d, window=window).cpu().numpy()
    before = flow.ssim_map(torch.from_numpy(img.copy()).to(_dev()), other_d, window=window).cpu().numpy()
    r = window // 2
    yy, xx = np.mgrid[0:h, 0:w]
    holds = np.zeros((n, h, w), bool)
    holds[1] = known[1] & (np.abs(yy - at[0]) <= r) & (np.abs(xx - at[1]) <= r)
    assert holds.sum() >= 2 and holds[1][at]
    assert np.array_equal(np.isnan(got), holds)
    assert np.array_equal(got[~holds].view(np.uint32), before[~holds].view(np.uint32))      # every other bit is unchanged
    assert np.array_equal(np.isnan(so.compute(a, m, dirty, other, ref, window)['map']), holds)     # the definition says the same
    stats = flow.ssim_stats(torch.from_numpy(dirty).to(_dev()), other_d, window=window)
    assert np.isnan(stats['sum'][1].item()) and not np.isnan(stats['sum'][0].item())
    assert stats['max'][1].item() == float(before[1][known[1] & ~holds[1]].max())           # a NaN is never the max
    assert stats['count'].tolist() == clean['records'][:, 0].tolist()
