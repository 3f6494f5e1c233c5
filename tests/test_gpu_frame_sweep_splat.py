"""GPU tier: the forward splat on every swept frame of tests/frame_sweep.py with W >= 4 (the gather path needs 4 columns), a launch of 6
images -- the frame's four and the first two again --, C = 1, 2, 3 and 5, with and without the mask channel, the occlusion rule on and
off, flow and data in fp32 and in fp16 (the fp16 up-conversions are what the oracle gets: exact).

  gather path (automatic)      values, mask channel, density and warped mask == oracle.apply_s_flow bit for bit; `_last_splat_stats` says
                               no image fell back and no tile left the exact path (tests/test_frame_sweep_host.py: no cell of these
                               inputs holds more than 64 records);
  forced passes                the same bits with set_splat_pass_images(1) and (3);
  two-pass path                set_splat_path(1): warped mask exact, values within rtol 2e-5 / atol 2e-5 * max |expected|;
  splat_sum                    bit for bit against its restatement (special_values.splat_sum_restated: the loops of
                               test_gpu_parity._splat_sum_reference, vectorised -- the CPU tier holds the two equal);
  splat_grad                   inside the per-element bound of tests/grad_oracle64.py.

Kernels reached.  `last_kernel_name()` names the LAST launch of a call, and a call on the gather path ends with the launch that walks
the list of images that fell back (empty here: the statistics say so) -- so the names seen, printed by the last test, are
  splat_fallback_kernel<1 | 2 | 3, float, float> and <2, _Float16, float>   gather path: splat_bin_kernel and splat_gather2_kernel<NC, MCH, TF,
                                                                            TO[, lean]> ran before it (C = 5: groups of 3 + 2 channels;
                                                                            the fp16 kernels take C = 2, other C are up-converted);
                                                                            also the last launch of splat_sum
  splat_finalize_kernel<0 | 1 | 2 | 3, float, float>                        the two-pass path (splat_fwd_kernel before it)
  splat_grad_kernel                                                         the backward (splat_grad_prep_kernel before it)
Every launch asserts the name of its route's last kernel; the fp16 launches at C = 2 a `_Float16` instantiation.
"""
import numpy as np
import pytest
import torch

import frame_sweep as fs
import grad_oracle64 as g64
import special_values as sv

pytestmark = pytest.mark.gpu
FRAMES = [(h, w) for h, w in fs.FRAMES if w >= 4]
N = 6
RTOL = 2e-5
SEEN = set()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tier needs a HIP device"
    from oflibpytorch_amd import _native
    _native.load_library()
    return torch.device('cuda', 0)


@pytest.fixture
def native():
    from oflibpytorch_amd import _native
    old = _native.collect_splat_stats
    _native.collect_splat_stats = True
    yield _native
    _native.collect_splat_stats = old
    _native.set_splat_path(0)
    _native.set_splat_pass_images(0)


def _inputs(h, w, c, half):
    """flow, data [4, c], weight mask, channel mask of the frame (NumPy; flow and data as the kernel reads them, up-converted)."""
    t = fs.content(h, w)
    flow = t["flow"].astype(np.float16).astype(np.float32) if half else t["flow"]
    data = np.ascontiguousarray((t["src"][:, :c] - np.float32(100)))      # integers in [-100, 155]: exact in fp16
    return flow, data, t["m1"], t["m2"]


def _first(got, exp):
    """None, or the first element whose bits differ: uint32 patterns, the sign of a zero included (no NaN in these inputs)."""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (got.shape, exp.shape, got.dtype, exp.dtype)
    same = got == exp if got.dtype == bool else got.view(np.uint32) == exp.view(np.uint32)
    bad = np.argwhere(~same)
    if not len(bad):
        return None
    idx = tuple(int(i) for i in bad[0])
    return "%d elements differ, the first at %s: got %r, expected %r" % (len(bad), idx, got[idx], exp[idx])


OPTIONS = [(mch, occ) for mch in (False, True) for occ in (True, False)]


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("c", [1, 2, 3, 5])
def test_forward_splat_on_every_frame(c, half, dev, native):
    from oracle import oracle
    for h, w in FRAMES:
        flow, data, wm, ca = _inputs(h, w, c, half)
        tf, td = (torch.from_numpy(fs.batch(a, N)).to(dev) for a in (flow, data))
        if half:
            tf, td = tf.half(), td.half()
            assert torch.equal(tf.float().cpu(), torch.from_numpy(fs.batch(flow, N))) and torch.equal(td.float().cpu(), torch.from_numpy(fs.batch(data, N)))
        twm, tca = (torch.from_numpy(fs.batch(a, N)).to(dev) for a in (wm, ca))
        native16 = half and c == 2        # the `_Float16` kernels (ofl_splat_tiled_f16) take 2 channels and give values + valid area only
        for mch, occ in OPTIONS:
            where = "frame %d x %d, C %d, %s, mask channel %d, occlusion %d" % (h, w, c, "fp16" if half else "fp32", mch, occ)
            kw = dict(weight_mask=twm, occlude=occ) if native16 else dict(weight_mask=twm, occlude=occ, want_density=True, want_warped=True)
            if mch:
                kw.update(chan_mask_a=tca, **(dict(want_valid=True) if native16 else dict(want_mask_chan=True)))
            dd = np.concatenate([data, (ca if mch else np.ones_like(ca))[:, None].astype(np.float32)], 1)
            ref, rwarped, rden = oracle.apply_s_flow(flow, dd, wm, occ, return_density=True)
            exp = dict(v=fs.batch(ref[:, :c], N), m=fs.batch(ref[:, c], N) if mch else None, den=fs.batch(rden, N), warped=fs.batch(rwarped, N))
            if native16:
                exp.update(den=None, warped=None, m=fs.batch(oracle.theta(ref[:, c]), N) if mch else None)

            def run(path=0, passes=0):
                native.set_splat_path(path)
                native.set_splat_pass_images(passes)
                native._last_splat_stats = None
                try:
                    out = native.splat_fwd(tf, td, **kw)
                    SEEN.add(native.last_kernel_name(demangle=False))
                finally:
                    native.set_splat_path(0)
                    native.set_splat_pass_images(0)
                st = native._last_splat_stats
                return dict(zip(("v", "m", "den", "warped"), (None if t is None else t.cpu().numpy() for t in out[:4]))), None if st is None else st.cpu().tolist()

            for passes in (0, 1, 3):
                got, st = run(0, passes)
                last = native.last_kernel_name(demangle=False)          # (the gather route ends with the walk over the images that fell back)
                assert "splat_fallback_kernel" in last and (not native16 or "DF16_" in last), "%s: the last launch was %s" % (where, last)
                assert st is not None and st[0] == 0 and st[1] == 0, "%s, passes %d: statistics %s" % (where, passes, st)
                for key in ("v", "m", "den", "warped"):
                    if exp[key] is not None:
                        msg = _first(got[key], exp[key])
                        assert msg is None, "%s, gather path (pass images %d), %s (n, [c,] y, x): %s" % (where, passes, key, msg)
            got, _ = run(1)
            assert "splat_finalize_kernel" in native.last_kernel_name(demangle=False), native.last_kernel_name(demangle=False)
            for key in ("warped", "m") if native16 else ("warped",):
                assert exp[key] is None or np.array_equal(got[key], exp[key]), "%s, two-pass path: %s" % (where, key)
            for key in ("v",) if native16 else ("v", "m", "den"):
                if exp[key] is not None:
                    np.testing.assert_allclose(got[key], exp[key], rtol=RTOL, atol=RTOL * float(np.abs(exp[key]).max()),
                                               err_msg="%s, two-pass path, %s" % (where, key))


@pytest.mark.parametrize("c", [1, 2, 3, 5])
def test_splat_sum_on_every_frame(c, dev, native):
    for h, w in FRAMES:
        flow, data, _, _ = _inputs(h, w, c, False)
        exp = fs.batch(sv.splat_sum_restated(flow, data), N)
        native._last_splat_stats = None
        out = native.splat_sum(torch.from_numpy(fs.batch(flow, N)).to(dev), torch.from_numpy(fs.batch(data, N)).to(dev), flow_sign=-1.0)
        SEEN.add(native.last_kernel_name(demangle=False))
        assert out is not None and "splat_fallback_kernel" in native.last_kernel_name(demangle=False), native.last_kernel_name(demangle=False)
        st = native._last_splat_stats.cpu().tolist()
        assert st[0] == 0 and st[1] == 0, "frame %d x %d: statistics %s" % (h, w, st)
        msg = _first(out.cpu().numpy(), exp)
        assert msg is None, "frame %d x %d, C %d, splat_sum (n, c, y, x): %s" % (h, w, c, msg)


@pytest.mark.parametrize("c", [1, 2, 3, 5])
def test_splat_grad_on_every_frame(c, dev, native):
    """Occlusion on and off, with and without the weight mask: the four combinations on every frame."""
    worst = 0.0
    for h, w in FRAMES:
        flow, data, wm, _ = _inputs(h, w, c, False)
        gout = np.ascontiguousarray(fs.content(h, w)["src"][:, 9 - c:] / np.float32(64) - np.float32(2))
        gden = np.ascontiguousarray(fs.content(h, w)["other"][:, 0])
        tf, td, tg, tgd, twm = (torch.from_numpy(a).to(dev) for a in (flow, data, gout, gden, wm))
        for occ in (True, False):
            for masked in (True, False):
                kw = dict(weight_mask=twm if masked else None, occlude=occ)
                out, _, den, _ = native.splat_fwd(tf, td, want_density=True, **kw)
                gd, gxy = native.splat_grad(tf, td, out, den, tg, grad_density=tgd, **kw)
                last = native.last_kernel_name(demangle=False)
                SEEN.add(last)
                assert "splat_grad_kernel" in last, last
                ref = g64.splat_grad(flow, data, out.cpu().numpy(), den.cpu().numpy(), gout, gden, wm if masked else None, occ, 1.0)
                for got, key in ((gd, 'grad_data'), (gxy, 'grad_xy')):
                    ex = g64.excess(got.cpu().numpy(), ref[key], g64.R['splat.' + key])
                    worst = max(worst, ex)
                    assert ex <= 1.0, "frame %d x %d, C %d, occlusion %d, mask %d, %s: error / bound %.4g" % (h, w, c, occ, masked, key, ex)
    print("C %d: worst error / bound %.4g over %d frames" % (c, worst, len(FRAMES)))


def test_zz_kernels_reached():
    """(runs last) prints the distinct kernels the launches of this file ended in; every launch has asserted its own above, so this
    holds nothing that depends on which tests of the file ran."""
    for raw in sorted(SEEN):
        print("splat sweep kernel:", raw)
