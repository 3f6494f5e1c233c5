"""The loss sweep's comparison code (a helper module, not a test): one launch of a fused loss kernel on a frame of
tests/frame_sweep.py against the family's NumPy oracle, with the bars of the family's own GPU test.

`run_*` launches through the package's bindings (`_photometric`, `_census`, `_smoothness`) on any device and returns NumPy arrays;
`check_*` runs and compares.  tests/test_gpu_loss_sweep_*.py call them on the HIP device, where `name_of` (the mangled name of the
last kernel) is asserted after every launch; tests/test_loss_sweep_host.py calls them on the CPU with the oracles' `fake_flow_*` entry
points in the bindings' place, and shows that they fail on a map off by one ulp in its last pixel and on a sum that lacks one block.

The bars (imported, not restated): maps bit for bit for photometric, census at q = 1 and smoothness without an image; `MAP_ULPS` of
tests/test_gpu_smoothness.py with an image, `POW_ULPS` of tests/test_gpu_census.py at the default q; counts exact; maxima exact (with a
guidance image: `MAX_ULPS`, the maximum being one of the map's own terms); float64 sums within count * 2^-52 relative (with a guidance
image plus 2^-22, as that file has it); the loss is the quotient of the call's own record; gradients within `grad_bound` of the float64
oracle and exactly +0 where the pixel is not known (smoothness: where no valid term reads it).  A failure names the frame, the variant
and the first element."""
import numpy as np
import torch

import census_oracle as cen
import frame_sweep as fs
import photometric_oracle as po
import smoothness_oracle as so
import test_gpu_census as tgc
import test_gpu_photometric as tgp
import test_gpu_smoothness as tgs

ALL = (0, 1, 2, 3)
F32 = np.float32


# ---- shared ---------------------------------------------------------------------------------------------------------------------------
def _named(name_of, part):
    if name_of is not None:
        name = name_of()
        assert part in name, "the launch reports %r, expected %r in it" % (name, part)


def _b(flag):
    return "Lb%dE" % int(bool(flag))


def _dev_of(dev, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _what(h, w, v, images):
    return "%d x %d, images %s, %s" % (h, w, list(images), ", ".join("%s %s" % kv for kv in sorted(v.items())))


def _first(bad):
    return tuple(int(i) for i in np.argwhere(bad)[0])


def none_of(bad, what, thing, got=None, want=None):
    """no element of `bad` is set; else the failure names the first"""
    if bad.any():
        at = _first(bad)
        raise AssertionError("%s: %s at %s%s" % (what, thing, at, "" if got is None else ": got %r, expected %r" % (got[at], want[at])))


def same_bits(got, want, what, thing):
    assert got.shape == want.shape and got.dtype == want.dtype == F32, (what, thing, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        at = _first(bad)
        raise AssertionError("%s: %s differs in %d elements, first at %s: got %r, expected %r" % (what, thing, int(bad.sum()), at, got[at], want[at]))


def sum_within(got, exact, count, what, thing, slack=0.0):
    """|got - exact| <= (slack + count 2^-52) exact: the terms are not negative, so this bounds any order of summation"""
    bound = (slack + count * 2.0 ** -52) * exact
    err = np.abs(got - exact)
    assert np.all(err <= bound), "%s: %s %s, exact %s, off by %s of the bound" % (what, thing, got.tolist(), exact.tolist(),
                                                                                  (err / np.maximum(bound, 1e-300)).tolist())


def grad_within(got, want, bound, zero, what, tally=None):
    """every element within its bound of the float64 oracle, finite, and exactly +0 where `zero`"""
    assert got.dtype == F32 and got.shape == want.shape, (what, got.shape, want.shape)
    none_of(np.broadcast_to(zero, got.shape) & (got.view(np.uint32) != 0), what, "the gradient is not +0 where it has to be,")
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bad = err > bound
    if bad.any():
        at = _first(bad)
        raise AssertionError("%s: the gradient at %s is %r, expected %r: %.3f of its bound" % (what, at, got[at], want[at], err[at] / bound[at]))
    if tally is not None:
        tally["grad"] = max(tally.get("grad", 0.0), float((err / bound).max()))
        tally["launches"] = tally.get("launches", 0) + 1


def _upstream(images):
    return np.asarray([fs.LOSS_UPSTREAM[i] for i in images], F32)


def _scale(up, count, dev):
    """upstream / count, formed as the bindings' callers form it: a float64 quotient rounded once"""
    return (torch.from_numpy(up).to(dev).double() / torch.from_numpy(np.ascontiguousarray(count)).to(dev)).float()


def _quotient(num, den):
    with np.errstate(invalid='ignore', divide='ignore'):
        return (num / den).astype(F32)


def _numpy(out):
    return {k: (None if x is None else x.cpu().numpy()) for k, x in out.items()}


# ---- photometric ----------------------------------------------------------------------------------------------------------------------
def photometric_operands(h, w, v, images=ALL):
    """(vectors, mask or None, img, other) as NumPy arrays, for the oracle and the launch alike"""
    t, sel = fs.loss_inputs(h, w), list(images)
    a = np.ascontiguousarray((t["flow16"] if v["half"] else t["flow"])[sel])
    mask = np.ascontiguousarray(t["mask"][sel]) if v["masked"] else None
    return (a, mask) + fs.images(t, v["u8"], v["chan"], sel)


def run_photometric(h, w, v, dev, images=ALL, backward=True, name_of=None):
    """dict(rec [n,8], map [n,h,w], loss [n], map_alone (a launch without records; with `name_of` only), grad [n,2,h,w] or None)"""
    from oflibpytorch_amd import _photometric as ph
    ops = _dev_of(dev, *photometric_operands(h, w, v, images))
    sign, eps = po.sign_of(v["ref"]), tgp.EPS
    out = dict(map_alone=None, grad=None)
    out["rec"], out["map"] = ph.flow_photometric(*ops, sign, eps, want_map=True)
    _named(name_of, "flow_photometric_finish_kernel")
    out["loss"] = ph.photometric(*ops, sign, eps)
    if name_of is not None:
        out["map_alone"] = ph.flow_photometric(*ops, sign, eps, want_map=True, want_record=False)[1]
        _named(name_of, "flow_photometric_kernelI" + _b(v["half"]) + _b(v["u8"]) + _b(False))
    if backward:
        out["grad"] = ph.flow_photometric_grad(*ops, sign, eps, _scale(_upstream(images), out["rec"][:, 0].cpu().numpy(), dev))
        _named(name_of, "flow_photometric_kernelI" + _b(v["half"]) + _b(v["u8"]) + _b(True))
    return _numpy(out)


def check_photometric(h, w, v, dev, images=ALL, backward=True, name_of=None, tally=None):
    a, mask, img, other = photometric_operands(h, w, v, images)
    want = po.compute(a, mask, img, other, v["ref"], tgp.EPS)
    got = run_photometric(h, w, v, dev, images, backward, name_of)
    what = _what(h, w, v, images)
    rec, n = got["rec"], len(images)
    assert rec.shape == (n, 8) and rec.dtype == np.float64, what
    same_bits(got["map"], want["map"], what, "the map (n, y, x)")                          # +0 where not known
    if got["map_alone"] is not None:
        same_bits(got["map_alone"], got["map"], what, "the map of a launch without records (n, y, x)")
    count, total = want["records"][:, 0], want["records"][:, 1]
    assert np.array_equal(rec[:, 0], count), "%s: count %s, expected %s" % (what, rec[:, 0].tolist(), count.tolist())
    assert np.array_equal(rec[:, 2], want["records"][:, 2]), "%s: max %s, expected %s" % (what, rec[:, 2].tolist(), want["records"][:, 2].tolist())
    assert not rec[:, 3:].any() and not np.signbit(rec[:, 3:]).any(), what
    sum_within(rec[:, 1], total, count, what, "sum")
    same_bits(got["loss"], _quotient(rec[:, 1], rec[:, 0]), what, "the loss against the quotient of its own record (n)")
    if backward:
        want_g, big_a = po.grad(a, mask, img, other, v["ref"], tgp.EPS, tuple(_upstream(images)))
        grad_within(got["grad"], want_g, po.grad_bound(want_g, big_a), ~want["known"][:, None], what, tally)
    return got


# ---- census ---------------------------------------------------------------------------------------------------------------------------
def _q(v):
    return 1.0 if v["q1"] else cen.Q


def run_census(h, w, v, dev, images=ALL, backward=True, name_of=None):
    from oflibpytorch_amd import _census as cs
    ops = _dev_of(dev, *photometric_operands(h, w, v, images))
    args = (cen.sign_of(v["ref"]), v["patch"], cen.THRESH, cen.EPS, _q(v))
    inst = "ILi%dE" % v["patch"] + _b(v["half"]) + _b(v["u8"])
    out = dict(map_alone=None, grad=None)
    out["rec"], out["map"] = cs.flow_census(*ops, *args, want_map=True)
    _named(name_of, "flow_census_finish_kernel")
    out["loss"] = cs.census(*ops, *args)
    if name_of is not None:
        out["map_alone"] = cs.flow_census(*ops, *args, want_map=True, want_record=False)[1]
        _named(name_of, "flow_census_kernel" + inst)
    if backward:
        out["grad"] = cs.flow_census_grad(*ops, *args, _scale(_upstream(images), out["rec"][:, 0].cpu().numpy(), dev))
        _named(name_of, "flow_census_grad_kernel" + inst)
    return _numpy(out)


def check_census(h, w, v, dev, images=ALL, backward=True, name_of=None, tally=None):
    a, mask, img, other = photometric_operands(h, w, v, images)
    want = cen.compute(a, mask, img, other, v["ref"], v["patch"], cen.THRESH, cen.EPS, _q(v))
    got = run_census(h, w, v, dev, images, backward, name_of)
    what = _what(h, w, v, images)
    rec, cmap, known = got["rec"], got["map"], want["known"]
    assert rec.shape == (len(images), 8) and rec.dtype == np.float64, what
    if v["q1"]:
        same_bits(cmap, want["map"], what, "the map (n, y, x)")
    else:
        none_of(~known & (cmap.view(np.uint32) != 0), what, "the map is not +0 where the pixel is not known,")
        ulps = np.abs(cmap.astype(np.float64) - want["map"]) / cen.ulp32(want["map"])
        none_of(known & ~((ulps <= tgc.POW_ULPS) & (cmap > 0)), what, "the map is off", cmap, want["map"])
        if tally is not None and known.any():
            tally["pow"] = max(tally.get("pow", 0.0), float(ulps[known].max()))
    if got["map_alone"] is not None:
        same_bits(got["map_alone"], cmap, what, "the map of a launch without records (n, y, x)")
    assert np.array_equal(rec[:, 0], want["records"][:, 0]), "%s: count %s, expected %s" % (what, rec[:, 0].tolist(), want["records"][:, 0].tolist())
    assert np.array_equal(rec[:, 3], want["records"][:, 3]), "%s: terms %s, expected %s" % (what, rec[:, 3].tolist(), want["records"][:, 3].tolist())
    tgc._check_record_against_own_map(rec, cmap, what)                                      # count, max, sum within count * 2^-52, the rest +0
    same_bits(got["loss"], _quotient(rec[:, 1], rec[:, 0]), what, "the loss against the quotient of its own record (n)")
    if backward:
        want_g, big_a = cen.grad(a, mask, img, other, v["ref"], v["patch"], cen.THRESH, cen.EPS, _q(v), tuple(_upstream(images)))
        grad_within(got["grad"], want_g, cen.grad_bound(want_g, big_a), ~known[:, None], what, tally)
    return got


# ---- smoothness -----------------------------------------------------------------------------------------------------------------------
def smoothness_operands(h, w, v, images=ALL):
    """(vectors, mask or None, guidance image or None)"""
    t, sel = fs.loss_inputs(h, w), list(images)
    a = np.ascontiguousarray((t["flow16"] if v["half"] else t["flow"])[sel])
    mask = np.ascontiguousarray(t["mask"][sel]) if v["masked"] else None
    img = None if v["kind"] is None else fs.images(t, v["kind"] == "u8", 3, sel)[0]
    return a, mask, img


def run_smoothness(h, w, v, dev, images=ALL, backward=True, name_of=None):
    from oflibpytorch_amd import _smoothness as sm
    ops = _dev_of(dev, *smoothness_operands(h, w, v, images))
    args = (v["order"], tgs.ALPHA, 1e-3)
    out = dict(grad=None)
    out["rec"], out["map"] = sm.flow_smoothness(*ops, *args, want_map=True)
    _named(name_of, "flow_smoothness_finish_kernel")
    out["loss"] = sm.smoothness(*ops, *args)
    if backward:
        terms = (out["rec"][:, 0] + out["rec"][:, 1]).cpu().numpy()
        out["grad"] = sm.flow_smoothness_grad(*ops, *args, _scale(_upstream(images), terms, dev))
        _named(name_of, "flow_smoothness_kernelILi%dELi%dE" % (v["order"], (None, "f32", "u8").index(v["kind"])) + _b(True))
    return _numpy(out)


def check_smoothness(h, w, v, dev, images=ALL, backward=True, name_of=None, tally=None):
    a, mask, img = smoothness_operands(h, w, v, images)
    want = so.compute(a, mask, img, v["order"], tgs.ALPHA, 1e-3)
    got = run_smoothness(h, w, v, dev, images, backward, name_of)
    what = _what(h, w, v, images)
    rec, smap, ref = got["rec"], got["map"], want["records"]
    assert rec.shape == (len(images), 8) and rec.dtype == np.float64, what
    if img is None:
        same_bits(smap, want["map"], what, "the map (n, y, x)")                            # +0 where no term is valid
        assert np.array_equal(rec[:, 4], ref[:, 4]), "%s: max %s, expected %s" % (what, rec[:, 4].tolist(), ref[:, 4].tolist())
        slack = 0.0
    else:
        bearing = want["x"]["ok"] | want["y"]["ok"]
        none_of(~bearing & (smap.view(np.uint32) != 0), what, "the map is not +0 where no term is valid,")
        assert (smap >= 0).all(), what
        d = np.abs(smap.view(np.int32).astype(np.int64) - want["map"].view(np.int32).astype(np.int64))
        none_of(bearing & (d > tgs.MAP_ULPS), what, "the map is off", smap, want["map"])
        if tally is not None:
            tally["map"] = max(tally.get("map", 0), int(d[bearing].max()) if bearing.any() else 0)
        assert np.array_equal(rec[:, 4].astype(F32).astype(np.float64), rec[:, 4]), what       # a float32 value
        assert tgs._ulps(rec[:, 4].astype(F32), ref[:, 4].astype(F32)).max() <= tgs.MAX_ULPS, "%s: max %s, expected %s" % (
            what, rec[:, 4].tolist(), ref[:, 4].tolist())
        slack = 2.0 ** -22
    assert np.array_equal(rec[:, :2], ref[:, :2]), "%s: counts %s, expected %s" % (what, rec[:, :2].tolist(), ref[:, :2].tolist())
    assert not rec[:, 5:].any(), what
    for k in (2, 3):
        sum_within(rec[:, k], ref[:, k], ref[:, k - 2], what, "sum_%s" % "xy"[k - 2], slack)
    same_bits(got["loss"], _quotient(rec[:, 2] + rec[:, 3], rec[:, 0] + rec[:, 1]), what, "the loss against the quotient of its own record (n)")
    if backward:
        want_g, big_a, read = so.grad(a, mask, img, v["order"], tgs.ALPHA, 1e-3, tuple(_upstream(images)))
        grad_within(got["grad"], want_g, so.grad_bound(want_g, big_a), ~read[:, None], what, tally)
    return got


# ---- a batch of two against an image on its own; two launches ---------------------------------------------------------------------------
def same_run(x, y, what, rows=(slice(None), slice(None))):
    """rows rx of run x carry the bits of rows ry of run y: record, map, loss and gradient"""
    rx, ry = rows
    for key in ("rec", "map", "loss", "grad"):
        if x[key] is None and y[key] is None:
            continue
        p, q = np.ascontiguousarray(x[key][rx]), np.ascontiguousarray(y[key][ry])
        none_of((p.view(np.uint8).reshape(p.shape + (-1,)) != q.view(np.uint8).reshape(q.shape + (-1,))).any(-1), what,
                "%s differs between the two launches" % key, p, q)
