"""GPU tier: the streaming kernels of the step at every size around one block's step.

These kernels are one-dimensional over h * w, 256 threads a block (read from the sources below), with a grid-stride loop.  What one
block covers in one step, E, differs (STEP below: pixels per thread and step of the vector form, and of the scalar form where there is one):
  flow_flags_kernel     VEC (h w % 4 == 0): 4 pixels x 4 groups in flight = 16 a thread, E = 4096; scalar: 1, E = 256
  flow_f16_kernel       4 pixels x 4 groups = 16 a thread, E = 4096 (h w % 4 == 0 only: other sizes are converted and take flow_flags_kernel)
  warp_valid_kernel     VEC (w % 4 == 0): 4 a thread, E = 1024; scalar: E = 256
  flow_extents_kernel   1 a thread, E = 256
  flow_error_kernel, flow_consistency_kernel, flow_epe_grad_kernel   quads with a guarded last one: 4 a thread, E = 1024
Swept per kernel: every h * w from 4 to E + 8 (E of its larger form) that a frame 2 x k or 3 x k has, and k * E - 3 ... k * E + 5 for
k = 2, 3 and each of its forms' E.  H >= 2 and W >= 2 throughout.

  flow_flags (fp32, fp16), flow_flags_host   oracle.flow_flags; non-finite, exact non-zero and sub-threshold non-zero values planted in
                                             the first element, the last element and the first element of the last vector, one per
                                             image of an otherwise all-zero batch; three more images carry a value under a False mask
                                             (5.0 at the last element, NaN at the first of the last vector, inf at the first element),
                                             which tells the masked bits from the unmasked ones
  warp_valid                                 oracle.theta of oracle.G of ones, both signs, with and without the mask
  flow_extents                               oracle.flow_extents
  flow_error                                 tests/flow_error_oracle.py: the map bit for bit, the counts and the maximum exactly, the
                                             float64 sums within count * 2^-52 relative (the bar of tests/test_gpu_flow_error.py)
  flow_consistency                           tests/consistency_oracle.py: maps bit for bit, counts and maximum exactly, sums as above
  flow_epe_grad                              flow_error_oracle.epe_grad in float64: both gradients within 4 float32 ulp (the bar of
                                             tests/test_gpu_flow_error.py), exactly 0 where the oracle is, grad_gt the negation bit for
                                             bit; the same on the one frame whose quads exceed the backward's largest grid (its loop)"""
import os
import re

import numpy as np
import pytest
import torch

import consistency_oracle as co
import flow_error_oracle as feo
import frame_sweep as fs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _threads(source, kernel):
    """Threads per block of a kernel, from its __launch_bounds__ (a number, or the kThreads constant of its file)."""
    with open(os.path.join(ROOT, 'oflibpytorch_amd', 'csrc', source)) as fh:
        text = fh.read()
    m = re.search(r"__launch_bounds__\((\w+)\)\s*(?:void\s+)?%s\(" % kernel, text)
    assert m, (source, kernel)
    tok = m.group(1)
    return int(tok) if tok.isdigit() else int(re.search(r"constexpr int %s = (\d+);" % tok, text).group(1))


# kernel -> (source, pixels per thread and block step of each of its forms, the larger first)
STEP = {"flow_flags_kernel": ("ofl_kernels.hip", (16, 1)), "flow_f16_kernel": ("ofl_kernels.hip", (16,)),
        "warp_valid_kernel": ("ofl_aux_kernels.hip", (4, 1)), "flow_extents_kernel": ("ofl_aux_kernels.hip", (1,)),
        "flow_error_kernel": ("ofl_metrics.hip", (4,)), "flow_consistency_kernel": ("ofl_consistency.hip", (4,)),
        "flow_epe_grad_kernel": ("ofl_metrics.hip", (4,))}


def _steps(kernel):
    """E of each form of a kernel: threads per block (from its source) x pixels per thread and step."""
    source, per_thread = STEP[kernel]
    return [_threads(source, kernel) * k for k in per_thread]


def _frame_of(hw):
    """The frame 2 x k or 3 x k of h w pixels (None: neither), so that both heights get every W % 4."""
    if hw % 6 == 0:
        return (3, hw // 3) if (hw // 6) % 4 < 2 else (2, hw // 2)
    if hw % 2 == 0:
        return (2, hw // 2)
    return (3, hw // 3) if hw % 3 == 0 and hw >= 6 else None


def _sizes_of(*forms):
    """The frames of the sweep for the block steps of one kernel's forms, or of several kernels' (the union of their ranges)."""
    vals = set()
    for es in forms:
        vals.update(range(4, max(es) + 9))
        for e in es:
            for k in (2, 3):
                vals.update(range(k * e - 3, k * e + 6))
    return [f for f in map(_frame_of, sorted(vals)) if f is not None]


def _sizes(*kernels):
    """The frames of the sweep for kernels that share a test."""
    return _sizes_of(*(_steps(kernel) for kernel in kernels))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tier needs a HIP device"
    from oflibpytorch_amd import _native
    _native.load_library()
    return torch.device('cuda', 0)


def test_the_sweep_covers_one_block_step_of_every_kernel():
    assert {k: _steps(k) for k in STEP} == {"flow_flags_kernel": [4096, 256], "flow_f16_kernel": [4096], "warp_valid_kernel": [1024, 256],
                                            "flow_extents_kernel": [256], "flow_error_kernel": [1024], "flow_consistency_kernel": [1024],
                                            "flow_epe_grad_kernel": [1024]}
    assert STEP["flow_epe_grad_kernel"][1] == (fs.loss_geometry()["metrics"]["grad_pixels"],)
    for kernel in STEP:
        sizes = _sizes(kernel)
        hw = {h * w for h, w in sizes}
        e = max(_steps(kernel))
        assert hw >= {v for v in range(4, e + 9) if v % 2 == 0 or (v % 3 == 0 and v >= 6)} and min(min(s) for s in sizes) >= 2
        assert {v for k in (2, 3) for v in range(k * e - 3, k * e + 6) if v % 2 == 0 or v % 3 == 0} <= hw
        assert {w % 4 for h, w in sizes if h == 2} == {0, 1, 2, 3} and {w % 4 for h, w in sizes if h == 3} == {0, 1, 2, 3}


# ---- the flag kernels ----------------------------------------------------------------------------------------------------------------
PLANTS = [float('nan'), float('inf'), 5.0, -0.25, 5e-4, -2e-4]          # non-finite, exact non-zero, non-zero under the threshold of 1e-3


IMAGES = 22


def _flag_case(h, w):
    """flow [22,2,h,w] and mask [22,h,w]: image i < 18 carries PLANTS[i % 6] at position (first, last, first of the last vector)[i // 6]
    in component i % 2 under a True mask; image 18 is all zero; images 19, 20, 21 carry 5.0 at the last element, NaN at the first element
    of the last vector and inf at the first element under a False mask."""
    hw = h * w
    spots = [0, hw - 1, (hw - 1) // 4 * 4]
    flow = np.zeros((IMAGES, 2, hw), np.float32)
    mask = np.ones((IMAGES, hw), bool)
    for i in range(18):
        flow[i, i % 2, spots[i // 6]] = PLANTS[i % 6]
    for i, (spot, val) in enumerate(((hw - 1, 5.0), (spots[2], float('nan')), (0, float('inf')))):
        flow[19 + i, i % 2, spot] = val
        mask[19 + i, spot] = False
    return flow.reshape(IMAGES, 2, h, w), mask.reshape(IMAGES, h, w)


@pytest.mark.parametrize("route", ["fp32", "fp16", "host", "host-fp16"])
def test_flag_kernels_at_every_size(route, dev):
    from oflibpytorch_amd import _native
    from oracle import oracle
    for h, w in _sizes("flow_flags_kernel", "flow_f16_kernel"):
        flow, mask = _flag_case(h, w)
        half = route.endswith("fp16")
        t = torch.from_numpy(flow)
        t = (t.half() if half else t).to(dev)
        ref_in = t.float().cpu().numpy()                                  # (5e-4 rounds in fp16: the oracle sees what the kernel sees)
        for m in (mask, None):
            want = oracle.flow_flags(ref_in, m).tolist()
            tm = None if m is None else torch.from_numpy(m).to(dev)
            if route.startswith("host"):
                got = _native.flow_flags_host(t, tm)
                if got is None:                                           # fp16 at h w % 4 != 0: no vector kernel, the caller takes flow_flags
                    assert half and (h * w) % 4 != 0, "%d x %d: the host route declined" % (h, w)
                    continue
            else:
                got = _native.flow_flags(t, tm).tolist()
            assert list(got) == want, "%s, %d x %d (h w = %d), %s: images %s differ: got %s, expected %s" % (
                route, h, w, h * w, "masked" if m is not None else "no mask", [i for i in range(IMAGES) if got[i] != want[i]], got, want)
        if half and route == "fp16":                                     # the conversion pass: every element, and the same word
            dst, flags = _native.flow_from_half(t, torch.from_numpy(mask).to(dev))
            assert torch.equal(dst.view(torch.int32), t.float().view(torch.int32)), "%d x %d: the fp32 copy" % (h, w)
            assert flags.tolist() == oracle.flow_flags(ref_in, mask).tolist(), "%d x %d: flow_from_half" % (h, w)


# ---- valid area, extents -------------------------------------------------------------------------------------------------------------
def _field(h, w, n=3):
    """A smooth flow of up to ~1.5 px (less across a 2- or 3-row frame), an identity stretch, integer shifts, a mask with holes."""
    rs = np.random.RandomState(17 * h + w)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    f = np.empty((n, 2, h, w), np.float32)
    for i in range(n):
        f[i, 0] = 1.5 * np.sin(x / 5.0 + i) + 0.4 * (y - 1)
        f[i, 1] = 0.6 * np.cos(x / 7.0 + 2 * i) + 0.2 * rs.randn(h, w)
    f[:, :, :, : w // 6] = 0.0
    f[:, 0, :, w // 3: w // 3 + 4] = np.round(f[:, 0, :, w // 3: w // 3 + 4])
    f.reshape(n, 2, -1)[:, :, -1] = (-0.5, 5e-4)                          # the last element: moves, and a component under the threshold
    m = rs.rand(n, h, w) > 0.15
    m.reshape(n, -1)[:, -1] = True
    return f, m


def test_warp_valid_at_every_size(dev):
    from oflibpytorch_amd import _native
    from oracle import oracle
    for h, w in _sizes("warp_valid_kernel"):
        f, m = _field(h, w)
        tf, tm = torch.from_numpy(f).to(dev), torch.from_numpy(m).to(dev)
        ones = np.ones((f.shape[0], 1, h, w), np.float32)
        for sign in (1.0, -1.0):
            area = oracle.theta(oracle.G(f * np.float32(sign), ones)[:, 0])
            for mask, tmask in ((m, tm), (None, None)):
                want = area if mask is None else area & mask
                got = _native.warp_valid(tf, tmask, sign, float(oracle.VALID_THRESHOLD)).cpu().numpy()
                assert np.array_equal(got, want), "%d x %d, sign %g, %s: first difference (n, y, x) %s" % (
                    h, w, sign, "masked" if mask is not None else "no mask", np.argwhere(got != want)[0].tolist())
        assert area.any() and not area.all()


def test_flow_extents_at_every_size(dev):
    from oflibpytorch_amd import _native
    from oracle import oracle
    for h, w in _sizes("flow_extents_kernel"):
        f, m = _field(h, w)
        m = m.copy()
        m[1] = False                                                      # an image without a valid pixel
        m[2].reshape(-1)[:-1] = False                                     # ... and one whose only valid pixel is the last
        tf, tm = torch.from_numpy(f).to(dev), torch.from_numpy(m).to(dev)
        for sign in (1.0, -1.0):
            for mask, tmask in ((m, tm), (None, None)):
                want = oracle.flow_extents(f, mask, sign)
                got = _native.flow_extents(tf, tmask, sign).cpu().numpy()
                ok = want[:, 4] > 0
                assert np.array_equal(got[:, 4], want[:, 4]) and np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), \
                    "%d x %d, sign %g, %s: got %s, expected %s" % (h, w, sign, "masked" if mask is not None else "no mask", got.tolist(), want.tolist())


# ---- the scores ------------------------------------------------------------------------------------------------------------------------
def _sums_within(got, exact, count, what):
    assert abs(got - exact) <= count * 2.0 ** -52 * exact, "%s: sum %.17g, exact %.17g" % (what, got, exact)


def test_flow_error_at_every_size(dev):
    import test_gpu_flow_error as tfe
    from oflibpytorch_amd import _native
    n = 2
    for h, w in _sizes("flow_error_kernel"):
        est, gt, em, gm = tfe._case.__wrapped__(n, h, w)
        ref = feo.score(est, gt, em, gm, tfe.THRESHOLDS)
        rec, emap = _native.flow_error(*(torch.from_numpy(a).to(dev) for a in (est, gt, em, gm)), tfe.THRESHOLDS, True)
        rec, emap = rec.cpu().numpy(), emap.cpu().numpy()
        where = "%d x %d (h w = %d)" % (h, w, h * w)
        bad = np.argwhere(emap.view(np.uint32) != ref['map'].view(np.uint32))
        assert not len(bad), "%s: the map differs first at (n, y, x) %s" % (where, bad[0].tolist())
        assert rec[:, 0].tolist() == ref['count'].tolist() and rec[:, 3:6].tolist() == ref['n_over'].tolist(), where
        assert rec[:, 7].tolist() == ref['n_fl'].tolist() and rec[:, 8:11].tolist() == ref['speed_count'].tolist(), where
        assert rec[:, 2].tolist() == ref['max'].tolist(), where
        for i in range(n):
            _sums_within(rec[i, 1], ref['sum'][i], ref['count'][i], where)
            for b in range(3):
                _sums_within(rec[i, 11 + b], ref['speed_sum'][i, b], ref['speed_count'][i, b], where)


def _epe_grad_frame(tfe, dev, n, h, w, est, gt, em, gm):
    """One launch of flow_epe_grad_kernel against the float64 oracle; returns the worst error in ulp."""
    from oflibpytorch_amd import _native
    where = "%d x %d (h w = %d)" % (h, w, h * w)
    count = feo.valid_of((n, h, w), em, gm).reshape(n, -1).sum(1)
    assert (count > 0).all(), where
    scale = (np.array([0.75, -2.0, 1.0], np.float32)[:n].astype(np.float64) / count).astype(np.float32)
    want = feo.epe_grad(est, gt, em, gm, scale)
    g_est, g_gt = _native.flow_epe_grad(*(torch.from_numpy(a).to(dev) for a in (est, gt, em, gm)), torch.from_numpy(scale).to(dev), True, True)
    assert 'flow_epe_grad_kernel' in _native.last_kernel_name()
    assert torch.equal(g_gt.view(torch.int32), (-g_est).view(torch.int32)), where
    got = g_est.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want) / ulp
    bad = np.argwhere((err > tfe.GRAD_ULPS) | ((want == 0) & (got != 0)))      # (a zero of either sign: scale * 0 / e)
    assert not len(bad), "%s: the gradient differs first at (n, c, y, x) %s: got %r, expected %r" % (
        where, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    return float(err.max()), bool((want == 0).any() and (want != 0).any()), want


def test_flow_epe_grad_at_every_size(dev):
    import test_gpu_flow_error as tfe
    n, worst, mixed = 2, 0.0, 0
    sizes = _sizes("flow_epe_grad_kernel")
    for h, w in sizes:
        e, m, _ = _epe_grad_frame(tfe, dev, n, h, w, *tfe._case.__wrapped__(n, h, w))
        worst, mixed = max(worst, e), mixed + m
    assert mixed == len(sizes)                                             # zeros (a hole, the tie with e = 0) and non-zeros side by side
    print("flow_epe_grad: worst %.3f ulp over %d sizes" % (worst, len(sizes)))


def test_flow_epe_grad_where_the_grid_loops(dev):
    """The one frame just over kMaxGradBlocks blocks of quads: the second round of the grid-stride loop (its last quad a partial one),
    which tests/test_loss_sweep_host.py proves from the constants."""
    import test_gpu_flow_error as tfe
    (state, h, w), = fs.loop_frames()["epe_grad"]
    walk = fs.epe_grad_walk(h, w)
    assert walk["rounds"] == 2 and 0 < walk["last"] < walk["stride"] and (h * w) % 4 != 0
    est, gt, em, gm = tfe._case.__wrapped__(1, h, w)
    e, m, want = _epe_grad_frame(tfe, dev, 1, h, w, est, gt, em, gm)
    assert m and (want.reshape(1, 2, -1)[:, :, 4 * walk["stride"]:] != 0).any()             # (the second round has a gradient to get wrong)
    print("flow_epe_grad, %d x %d: worst %.3f ulp" % (h, w, e))


@pytest.mark.parametrize("ref", ["s", "t"])
def test_flow_consistency_at_every_size(ref, dev):
    from oflibpytorch_amd import _consistency
    n, alpha, beta = 2, co.ALPHA, co.TABLE_BETA
    seen = np.zeros(2, np.int64)
    for h, w in _sizes("flow_consistency_kernel"):
        a, back, am, bm = co.case.__wrapped__(n, h, w, ref, 0.1)
        want = co.check(a, back, am, bm, ref, alpha, beta)
        err, cons, known, rec = _consistency.flow_consistency(*(torch.from_numpy(x.copy()).to(dev) for x in (a, back, am, bm)),
                                                              -1.0 if ref == 's' else 1.0, alpha, beta)
        where = "%s, %d x %d (h w = %d)" % (ref, h, w, h * w)
        err, rec = err.cpu().numpy(), rec.cpu().numpy()
        bad = np.argwhere(err.view(np.uint32) != want['error'].view(np.uint32))
        assert not len(bad), "%s: the error map differs first at (n, y, x) %s" % (where, bad[0].tolist())
        assert np.array_equal(known.cpu().numpy(), want['known']) and np.array_equal(cons.cpu().numpy(), want['consistent']), where
        r = want['records']
        assert rec[:, 0].tolist() == r[:, 0].tolist() and rec[:, 1].tolist() == r[:, 1].tolist() and rec[:, 3].tolist() == r[:, 3].tolist(), where
        for i in range(n):
            _sums_within(rec[i, 2], r[i, 2], r[i, 0], where)
            _sums_within(rec[i, 4], r[i, 4], r[i, 1], where)
        seen += [int(want['known'].sum()), int((want['known'] & ~want['consistent']).sum())]
    assert seen[0] > 0 and seen[1] > 0                                    # (known pixels of both kinds over the sweep)
