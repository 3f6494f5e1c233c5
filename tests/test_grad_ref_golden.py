"""CPU tier: tests/grad_ref.py (the reference's differentiable op sequences restated with torch ops) against the fixtures the
reference itself produced -- every grads.* case, the float / integer / broadcast track_pts and Flow.track cases, and the
get_padding / get_flow_padding cases.  Forward values and masks bit for bit, gradients within case_runner.GRAD_RTOL, padding
lists exactly.  This is what lets tests/test_gpu_gradients.py use grad_ref as the reference at frame sizes where no fixture
exists."""
import numpy as np
import pytest
import torch

import case_runner
import codec
import grad_ref
from conftest import golden_ids
from grad_ref import RFlow

GRAD_OPS = ('grad_apply_flow', 'grad_gfud', 'grad_track_pts', 'grad_Flow.apply', 'grad_Flow.switch_ref', 'grad_Flow.invert',
            'grad_Flow.combine_with', 'grad_Flow.combine')


def _t(a):
    return None if a is None else torch.tensor(np.asarray(a))


def _leaf(i, k):
    return _t(i[k]).clone().requires_grad_()


def _exact(got, exp, what):
    got = got.detach().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    bad = ~((got == exp) | (np.isnan(got) & np.isnan(exp))) if exp.dtype.kind == 'f' else got != exp
    assert not bad.any(), "%s: %d of %d values differ" % (what, int(bad.sum()), bad.size)


def _grad(got, exp, what):
    got = torch.zeros(exp.shape) if got is None else got
    g = got.detach().numpy()
    assert g.shape == exp.shape and g.dtype == exp.dtype, (what, g.shape, exp.shape)
    scale = float(np.max(np.abs(exp))) if exp.size else 0.0
    err = float(np.max(np.abs(g.astype(np.float64) - exp.astype(np.float64)))) if exp.size else 0.0
    assert err <= case_runner.GRAD_RTOL * max(scale, 1e-6), "%s: max |diff| %.3g vs gradient scale %.3g" % (what, err, scale)


def test_every_grads_fixture_is_covered():
    assert len(golden_ids(*GRAD_OPS)) == 23 == len(golden_ids(group='grads'))


@pytest.mark.parametrize("cid", golden_ids(*GRAD_OPS))
def test_grad_ref_against_the_grads_fixtures(cid, golden):
    case = golden.cases[cid]
    i, exp = golden.arrays(case)
    a, op = case["args"], case["op"]
    if op == 'grad_apply_flow':
        fv, tv = _leaf(i, "flow"), _leaf(i, "target")
        out = grad_ref.apply_flow(fv, tv, a["ref"], _t(i.get("mask")))
        (out * _t(i["w_out"])).sum().backward()
        _grad(fv.grad, exp["g_flow"], "g_flow")
        _grad(tv.grad, exp["g_target"], "g_target")
        return
    if op == 'grad_gfud':
        xv, yv, dv = _leaf(i, "x"), _leaf(i, "y"), _leaf(i, "data")
        od, oden = grad_ref.grid_from_unstructured_data(xv, yv, dv, _t(i.get("mask")))
        ((od * _t(i["w_data"])).sum() + (oden * _t(i["w_density"])).sum()).backward()
        for k, v in (("g_x", xv), ("g_y", yv), ("g_data", dv)):
            _grad(v.grad, exp[k], k)
        return
    if op == 'grad_track_pts':
        fv, pv = _leaf(i, "flow"), _leaf(i, "pts")
        out = grad_ref.track_pts(fv, a["ref"], pv)
        _exact(out, exp["out"], "out")
        (out * _t(i["w_out"])).sum().backward()
        _grad(fv.grad, exp["g_flow"], "g_flow")
        _grad(pv.grad, exp["g_pts"], "g_pts")
        return
    fa, fb = _leaf(i, "f1"), _leaf(i, "f2")
    m1, m2 = _t(i["m1"]), _t(i["m2"])
    if op == 'grad_Flow.apply':
        out = RFlow(fa, a["ref"], m1).apply(RFlow(fb, a["target_ref"], m2))
    elif op == 'grad_Flow.switch_ref':
        out = RFlow(fa, a["ref"], m1).switch_ref()
    elif op == 'grad_Flow.invert':
        out = RFlow(fa, a["ref"], m1).invert()
    elif op == 'grad_Flow.combine_with':
        out = RFlow(fa, a["ref"], m1).combine_with(RFlow(fb, a["ref"], m2), a["mode"])
    else:
        out = RFlow(fa, a["self_ref"], m1).combine(RFlow(fb, a["other_ref"], m2), a["mode"], a["ref"])
    _exact(out.vecs, exp["vecs"], "vecs")
    _exact(out.mask, exp["mask"], "mask")
    (out.vecs * _t(i["w_out"])).sum().backward()
    _grad(fa.grad, exp["g_f1"], "g_f1")
    _grad(fb.grad, exp["g_f2"], "g_f2")


@pytest.mark.parametrize("cid", golden_ids('track_pts', 'Flow.track'))
def test_grad_ref_track_pts_against_the_fixtures(cid, golden):
    case = golden.cases[cid]
    i, exp = golden.arrays(case)
    a = case["args"]
    fv = _t(i["flow_raw"]) if "flow_raw" in i else \
        _t(codec.decode_affine(i["flow__params"], i["flow__delta"], i["flow__esc"])[None])
    pts = _t(i["pts"])
    if case["op"] == 'track_pts':
        _exact(grad_ref.track_pts(fv, a["ref"], pts, bool(a["int_out"])), exp["out"], "out")
        return
    fl = RFlow(fv, a["ref"], _t(i["m"]))
    if a.get("batch"):
        fl = RFlow(fl.vecs.repeat(a["batch"], 1, 1, 1), fl.ref, fl.mask.repeat(a["batch"], 1, 1))
    _exact(fl.track(pts, bool(a["int_out"])), exp["out"], "out")


@pytest.mark.parametrize("cid", golden_ids('Flow.get_padding', 'get_flow_padding'))
def test_grad_ref_padding_against_the_fixtures(cid, golden):
    case = golden.cases[cid]
    i, _ = golden.arrays(case)
    a = case["args"]
    if case["op"] == 'Flow.get_padding':
        got = RFlow(_t(i["f"]), a["ref"], _t(i["m"])).get_padding(a["item"])
    else:
        v = _t(i["flow_raw"])
        got = grad_ref.flow_padding(v, a["ref"])
        if a["layout"] == 'chw':
            got = got[0]
        elif a["layout"] == 'hwc_np':
            got = grad_ref.flow_padding(v[1:2], a["ref"])[0]
    assert got == a["padding"], (got, a["padding"])
