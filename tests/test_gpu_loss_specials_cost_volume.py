"""GPU tier of tests/loss_specials.py for the cost volume (ofl_cost_volume.hip) at named sample positions and on NaN,
+-inf and +-FLT_MAX, beside tests/test_gpu_loss_specials.py and with its helpers.  The cases are `loss_specials.cost_volume_case`: 20 x 28
at r = 1, 37 x 53 at r = 4 with one channel more than a staged chunk, 17 x 33 at r = 1 with the plants on both sides of the tile edges;
four images each (mixed pool, +FLT_MAX only, NaN only, clean).

  (a) the volume, d feat and d W equal `cost_volume_oracle.compute` / `grads` bit for bit on every variant (the payload of a NaN exempt)
  (b) an element none of whose inputs differs from the finite variant carries the finite variant's bits; the sets come from the taps
  (c) the clean image carries the finite variant's bits
  (d) a pixel with a vector that is not finite is not usable: W' and d W are +0 there, the bits the oracle's
  (e) through backward() on 'unsampled', 'vectors' and 'finite': d feat, d other and d flow are finite, d flow is +0 at every pixel that
      is not usable, d other is 0 at the planted pixels, and all three are within 2e-4 of their scale of the float64 autograd of the
      definition evaluated with the planted values replaced by 0 -- by the definition they are inputs of no usable sample
  (f) through backward() on 'feat', 'other' and 'upstream' (the one public path that hands the warp's gradient kernels an upstream
      gradient that is not finite): the clean image keeps its bits, every element of d feat, d other and d flow none of whose inputs
      differs keeps them too, d flow is +0 at every pixel that is not usable, and the mixed and the NaN image do hold a non-finite element

tests/test_loss_specials_host.py shows on the CPU that no case is empty of any of this."""
import numpy as np
import pytest

import loss_specials as ls
from test_gpu_loss_specials import _np, _t

gpu = pytest.mark.gpu
N = ls.N
FRAMES = ls.cv_frames()
IDS = ["%dx%d-r%d-C%d" % f for f in FRAMES]


def _kernels(case):
    """{volume, d feat, d W} of the three launches, each under the name it must report"""
    from oflibpytorch_amd import _cost_volume, _native
    sign, r = ls.sign_of(case['ref']), case['radius']
    ops = (_t(case['a']), _t(case['mask']), _t(case['feat']), _t(case['other']))
    vol = _cost_volume.flow_cost_volume(*ops, sign, r)
    assert 'flow_cost_volume_kernel' in _native.last_kernel_name()
    d_feat, none = _cost_volume.flow_cost_volume_grad(*ops, sign, r, _t(case['g']), want_warped=False)
    assert none is None and 'flow_cost_volume_grad_kernel' in _native.last_kernel_name()
    none, d_w = _cost_volume.flow_cost_volume_grad(*ops, sign, r, _t(case['g']), want_feat=False)
    assert none is None and 'flow_cost_volume_grad_kernel' in _native.last_kernel_name()
    return {'volume': _np(vol), 'd_feat': _np(d_feat), 'd_w': _np(d_w)}


def _backward(case):
    """{d feat, d other, d flow} of `backward()` with the case's upstream gradient"""
    from oflibpytorch_amd import _cost_volume, _native
    v, ft, ot = _t(case['a'], grad=True), _t(case['feat'], grad=True), _t(case['other'], grad=True)
    vol = _cost_volume.cost_volume(v, _t(case['mask']), ft, ot, ls.sign_of(case['ref']), case['radius'])
    assert vol.requires_grad and type(vol.grad_fn).__name__ == "CostVolumeFnBackward"
    assert 'flow_cost_volume_kernel' in _native.last_kernel_name()
    vol.backward(_t(case['g']))
    assert 'flow_cost_volume_gate_kernel' in _native.last_kernel_name()           # the last launch of the backward: the select of d flow
    return {'d_feat': _np(ft.grad), 'd_other': _np(ot.grad), 'd_flow': _np(v.grad)}


def _count(x):
    return (~np.isfinite(x)).reshape(N, -1).sum(1).tolist()


@gpu
@pytest.mark.parametrize("ref", ls.REFS)
@pytest.mark.parametrize("h,w,radius,c", FRAMES, ids=IDS)
def test_volume_and_gradient_kernels(h, w, radius, c, ref):
    """(a) to (d); the finite variant also with fp16-stored vectors at 20 x 28"""
    finite_run = {}
    configs = [(v, False) for v in ls.CV_VARIANTS] + ([('finite', True)] if (h, w) == (20, 28) else [])
    for variant, half in configs:
        case = ls.cost_volume_case(h, w, ref, variant, c, half)
        what = "cost volume %d x %d r %d C %d '%s' %s half %s" % (h, w, radius, c, ref, variant, half)
        got = _kernels(case)
        ls.check_cost_volume_kernels(case, got, None if variant == 'finite' else finite_run[half], what)
        print("%s: elements that are not finite: volume %s, d feat %s, d W %s" % (what, _count(got['volume']), _count(got['d_feat']),
                                                                                   _count(got['d_w'])))
        if variant == 'finite':
            finite_run[half] = got


@gpu
@pytest.mark.parametrize("ref", ls.REFS)
@pytest.mark.parametrize("h,w,radius,c", FRAMES, ids=IDS)
def test_backward_keeps_what_no_usable_pixel_samples_out_of_every_gradient(h, w, radius, c, ref):
    """(e).  Before the select of 3.24 existed, d flow at a pixel that is not usable was 0 * tap: NaN for a tap of `other` that is not
    finite, on the input whose forward is finite."""
    for variant in ('finite', 'unsampled', 'vectors'):
        case = ls.cost_volume_case(h, w, ref, variant, c)
        what = "cost volume backward %d x %d r %d C %d '%s' %s" % (h, w, radius, c, ref, variant)
        errs = ls.check_cost_volume_backward(case, _backward(case), None, what)
        print(what + ": " + ", ".join("%s max error %.3e of a scale %.3e" % ((k,) + v) for k, v in errs.items()))


@gpu
@pytest.mark.parametrize("ref", ls.REFS)
@pytest.mark.parametrize("h,w,radius,c", FRAMES, ids=IDS)
def test_backward_isolates_what_a_special_reaches(h, w, radius, c, ref):
    """(f), and 'upstream': the one public path that hands the warp's gradient kernels an upstream gradient that is not finite"""
    fin = _backward(ls.cost_volume_case(h, w, ref, 'finite', c))
    for variant in ('feat', 'other', 'upstream'):
        case = ls.cost_volume_case(h, w, ref, variant, c)
        what = "cost volume backward %d x %d r %d C %d '%s' %s" % (h, w, radius, c, ref, variant)
        got = _backward(case)
        ls.check_cost_volume_backward(case, got, fin, what)
        print("%s: elements that are not finite: d feat %s, d other %s, d flow %s" % (what, _count(got['d_feat']), _count(got['d_other']),
                                                                                      _count(got['d_flow'])))
