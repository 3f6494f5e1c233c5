"""GPU tier of tests/loss_specials.py for the SSIM loss (ofl_ssim.hip) at named sample positions and on NaN, +-inf and
+-FLT_MAX, beside tests/test_gpu_loss_specials.py and with its helpers.  The cases are `loss_specials.ssim_case`: window 3 at 37 x 53,
windows 5 and 7 at 67 x 131 (four tiles + 3 by two tiles + 3 of the 64 x 16 tile), window 3 at 17 x 65 with the plants on both sides of
the tile edges; four images each (mixed pool, +FLT_MAX only, NaN only, clean); specials in `other`, in `img`, in the vectors; the finite
variant also as uint8 images, as C = 1 and with fp16-stored vectors.  The bars are `loss_specials.check_ssim`:

  forward    the map equals the oracle's on the terms of special_values.same_bits and is +0 where not known
  records    count and [3] exact, sum and maximum those of the call's own map by the rule of 3.16, the loss the quotient of the record
  isolation  a known pixel none of whose window pixels reads a planted element (the readers dilated by R; by 2 R for the gradient)
             carries the finite variant's bits; the clean image carries them everywhere
  gradient   exactly +0 where not known (a vector of its own that is not finite included); the oracle's class where its value or A is
             not finite; within 2^-22 A + ulp32(want) elsewhere; not 0 at the named border pixels of the finite variant

tests/test_loss_specials_host.py shows on the CPU that no case is empty of any of this."""
import numpy as np
import pytest

import loss_specials as ls
import ssim_oracle as sso
from test_gpu_loss_specials import _np, _t, _up

gpu = pytest.mark.gpu
N = ls.N
# (variant, channels, uint8 images, fp16-stored flow)
CONFIGS = [('finite', 3, False, False), ('finite', 3, True, False), ('finite', 3, False, True), ('finite', 1, False, False),
           ('other', 3, False, False), ('img', 3, False, False), ('vectors', 3, False, False)]


def _launches(case, window, upstream=None):
    """(record, map, loss, gradient) of one case, each launch under the name it must report"""
    from oflibpytorch_amd import _native, _ssim
    sign = ls.sign_of(case['ref'])
    mask, ti, to = _t(case['mask']), _t(case['img']), _t(case['other'])
    extra = (window, sso.C1, sso.C2)
    rec, smap = _ssim.flow_ssim(_t(case['a']), mask, ti, to, sign, *extra, want_map=True)
    assert 'flow_ssim_finish_kernel' in _native.last_kernel_name()
    up = _up() if upstream is None else upstream
    if case['half']:                                            # an fp16 leaf: the loss and the gradient through the bindings
        loss = _ssim.ssim(_t(case['a']), mask, ti, to, sign, *extra)
        grad = _ssim.flow_ssim_grad(_t(case['a']), mask, ti, to, sign, *extra, (up.double() / rec[:, 0]).float())
    else:
        v = _t(case['a'], grad=True)
        loss = _ssim.ssim(v, mask, ti, to, sign, *extra)
        assert loss.requires_grad
        loss.backward(up)
        grad = v.grad
    assert 'flow_ssim_grad_kernel' in _native.last_kernel_name()
    return _np(rec), _np(smap), _np(loss), _np(grad)


@gpu
@pytest.mark.parametrize("ref", ls.REFS)
@pytest.mark.parametrize("h,w,window", ls.SSIM_FRAMES, ids=lambda v: str(v))
def test_ssim(h, w, window, ref):
    finite_run, worst = {}, 0.0
    for variant, c, u8, half in CONFIGS:
        case = ls.ssim_case(h, w, ref, variant, c, half, u8)
        what = "ssim %d x %d window %d '%s' %s C %d u8 %s half %s" % (h, w, window, ref, variant, c, u8, half)
        rec, smap, loss, grad = _launches(case, window)
        key = (c, u8, half)
        ratio, share = ls.check_ssim(case, window, rec, smap, loss, grad, None if variant == 'finite' else finite_run[key], what)
        worst = max(worst, ratio)
        print("%s: sums %s max %s; gradient %.3f of its bound, %.3f of the non-zero elements by class" % (what, rec[:, 1], rec[:, 2], ratio, share))
        if variant == 'finite':
            finite_run[key] = (rec, smap, grad)
    print("ssim %d x %d window %d '%s': largest gradient error %.3f of the bound 2^-22 A + ulp32" % (h, w, window, ref, worst))


@gpu
@pytest.mark.parametrize("ref", ls.REFS)
def test_ssim_gradient_under_an_upstream_gradient_that_is_not_finite(ref):
    """Upstream (NaN, +inf, 1, 0.5) on the finite variant: images 0 and 1 have a gradient of exactly +0 where not known and of the
    oracle's class where known; images 2 and 3 keep the bits of their own images run singly with that upstream."""
    import torch
    from oflibpytorch_amd import _native, _ssim
    h, w, window = ls.SSIM_FRAMES[0]
    case = ls.ssim_case(h, w, ref, 'finite')
    up = (float('nan'), float('inf'), 1.0, 0.5)
    _, _, _, grad = _launches(case, window, torch.tensor(up, device=_t(case['mask']).device))
    res = sso.compute(case['a'], case['mask'], case['img'], case['other'], ref, window)
    want, big_a = sso.grad(case['a'], case['mask'], case['img'], case['other'], ref, window, upstream=up, res=res)
    zero = ~np.broadcast_to(res['known'][:, None], grad.shape)
    ls.check_gradient(grad, want, big_a, zero, sso.ulp32, "upstream %s" % (up,))
    assert np.isnan(grad[0][~zero[0]]).all() and (~np.isfinite(grad[1][~zero[1]])).all()
    sign = ls.sign_of(ref)
    for i in (2, 3):
        one = slice(i, i + 1)
        v = _t(case['a'][one], grad=True)
        _ssim.ssim(v, _t(case['mask'][one]), _t(case['img'][one]), _t(case['other'][one]), sign, window, sso.C1, sso.C2).backward(
            torch.tensor(up[one], device=v.device))
        assert 'flow_ssim_grad_kernel' in _native.last_kernel_name()
        assert np.array_equal(_np(v.grad)[0].view(np.uint32), grad[i].view(np.uint32)), i
        assert np.isfinite(grad[i]).all() and np.abs(grad[i]).max() > 0
