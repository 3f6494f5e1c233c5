"""GPU tier: the gather splat (`ofl_splat_tiled_f32`) at every cell length where its ordering changes mechanism, in
both of its launches, with fp16 flows and data, where it folds, on rough 1080p flows, and on the reference's masked 's' known-answer
test.

tests/splat_cells.py builds flows in which chosen destination cells receive exactly k records from horizontally adjacent pixels of
different lanes and of two subtiles (their chains arrive out of raster order), with data whose class sums change with the order of
their additions; tests/test_splat_cells_host.py pins both on the CPU.  Wherever the in-order path runs, every value, density, mask
channel and warped mask must equal the C oracle's bit for bit.  Bands the first launch marks on its redo list are summed with LDS
float atomics: there values may differ within rtol 2e-5 / atol 2e-5 * max|expected|, and nowhere else.

The rows of DESIGN.md 3.2's ordering table the k sweep targets (splat_cells.mechanism; 3 data channels / 1-2):
  k = 1, 2               nothing orders them (a + b from +0 commutes): phase S skipped
  k = 3, 4               5-comparator network, chain re-linked
  k = 5, 6 / 5 ... 8     sorting network in one lane's registers, class sums written over part A
  k = 7 / 9 ... 64       a wave per cell (sp2_order_big_cell); in the second launch the whole block (sp2_big_cells_block)
  the same k in tiles of more records than the LDS holds: bands planned from exact row counts, second launch (REDO)
  k = 65, 80, a row pair over capacity: band marked, LDS float atomics
"""
import os
import types

import numpy as np
import pytest
import torch

import splat_cells as sc

pytestmark = pytest.mark.gpu

# A library built with other compile-time switches (tools/build_variant.sh, loaded through OFL_HIP_LIB) promises the same bits through
# other launches: the assertions on the call's statistics and redo list, which describe the default build's route, are left out for it.
VARIANT = bool(os.environ.get("OFL_HIP_LIB"))
RTOL = 2e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tier needs a HIP device"
    from oflibpytorch_amd import _native
    _native.load_library()
    assert _native.splat_tile_geometry()[:2] == (sc.TW, sc.TH)
    return torch.device('cuda', 0)


@pytest.fixture
def native():
    """_native with the whole workspace of the last gather splat kept (_last_splat_ws: statistics and redo list)."""
    from oflibpytorch_amd import _native
    old = _native.collect_splat_stats
    _native.collect_splat_stats = 2
    yield _native
    _native.collect_splat_stats = old


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _splat(native, dev, fr, data, ca, c, occlude, mask_chan, sign=1.0):
    """Two identical calls of _native.splat_fwd; flow and data are handed over multiplied by `sign` with flow_sign = data_sign = sign,
    so that the splat is the frame's whichever the sign.  -> [dict(v, m, den, warped, stats, ws)] per call."""
    f = torch.from_numpy(fr.flow * np.float32(sign)).to(dev)
    d = torch.from_numpy(np.ascontiguousarray(data[:, :c] * np.float32(sign))).to(dev)
    kw = dict(flow_sign=sign, data_sign=sign, weight_mask=torch.from_numpy(fr.on).to(dev), occlude=occlude, want_density=True,
              want_warped=True)
    if mask_chan:
        kw.update(chan_mask_a=torch.from_numpy(ca).to(dev), want_mask_chan=True)
    runs = []
    for _ in range(2):
        out = native.splat_fwd(f, d, **kw)
        runs.append(dict(v=out[0].cpu().numpy(), m=None if out[1] is None else out[1].cpu().numpy(), den=out[2].cpu().numpy(),
                         warped=out[3].cpu().numpy(), stats=native._last_splat_stats.cpu().tolist(),
                         ws=native._last_splat_ws.cpu().numpy()))
    return runs


def _expected(fr, data, ca, c, occlude, mask_chan):
    from oracle import oracle
    dd = data[:, :c]
    if mask_chan:
        dd = np.concatenate([dd, ca[:, None].astype(np.float32)], 1)
    ref, warped, den = oracle.apply_s_flow(fr.flow, dd, fr.on, occlude, return_density=True)
    return dict(v=ref[:, :c], m=ref[:, c] if mask_chan else None, den=den, warped=warped)


def _differs(got, exp):
    """[n, h, w]: the pixels where any value, the density, the mask channel or the warped mask differs in any bit."""
    d = (_bits(got["v"]) != _bits(exp["v"])).any(1) | (_bits(got["den"]) != _bits(exp["den"])) | (got["warped"] != exp["warped"])
    if exp["m"] is not None:
        d |= _bits(got["m"]) != _bits(exp["m"])
    return d


def _by_k(diff, info):
    """{k: cells} of the cells that serve the pixels that differ (None: a medium cell; '-': no cell of the frame)."""
    out = {}
    for b, y, x in np.argwhere(diff):
        key = sc.cell_of_pixel(b, y, x)
        out.setdefault(info["k_of"].get(key, "-"), set()).add(key)
    return {k: len(v) for k, v in sorted(out.items(), key=lambda kv: str(kv[0]))}


def _units(native, r, fr):
    return sc.redo_units(r["ws"], fr.n, fr.h, fr.w, native.splat_tile_geometry()[2])


# ---- 2. the k sweep, (a) in tiles that fit (first launch), (b) in tiles of more records than the LDS holds (second launch) ----------
SWEEP = ([(c, mch, occ, 1.0) for c in (1, 2, 3) for mch in (False, True) for occ in (True, False)]   # (data channels, mask channel,
         + [(4, True, True, 1.0), (5, True, False, 1.0), (3, True, True, -1.0)])                    #  occlude_zero_flow, signs)


@pytest.mark.parametrize("launch", ["first", "second"])
@pytest.mark.parametrize("c,mch,occ,sign", SWEEP)
def test_every_cell_length_is_bit_exact(launch, c, mch, occ, sign, dev, native):
    """Every k of the sweep (4 cells of each per tile in 'first', 1 among ~240 medium cells in 'second') against the oracle, bit for
    bit: values, density, mask channel (holes in some tiles, none in their neighbours, one on a source scanned by a tile whose record
    lands in the next), warped mask; twice, with the same bits.  C = 4 / 5 run through channel groups of 3."""
    fr, info, data, ca = sc.make(launch)
    # the sweep reaches every row of the ordering table for each channel group (k = 1, 2 | 3, 4 | 5 .. 6 / 8 | 7 / 9 .. 64)
    for nc in sorted({min(c - c0, 3) for c0 in range(0, c, 3)}):
        assert {sc.mechanism(k, nc) for k in sc.K_SWEEP} == {"none", "network5", "lane-network", "wave"}
    assert sc.record_counts(fr.flow, fr.on, occ) == fr.counts(occ)
    runs = _splat(native, dev, fr, data, ca, c, occ, mch, sign)
    exp = _expected(fr, data, ca, c, occ, mch)
    for r in runs:
        diff = _differs(r, exp)
        assert not diff.any(), "%s launch, C=%d: %d pixels differ from the oracle; cells that serve them, by k: %s" % (
            launch, c, int(diff.sum()), _by_k(diff, info))
    for key in ("v", "m", "den", "warped"):
        if runs[0][key] is not None:
            assert _same(runs[0][key], runs[1][key]), "run to run: %s" % key
    if VARIANT:
        return
    for r in runs:
        st, units = r["stats"], _units(native, r, fr)
        assert st[0] == 0 and st[1] == 0 and st[2] == 0, st        # no image on the two-pass path, no band folded
        if launch == "first":
            assert st[3] == 0 and units == [], st                 # every tile summed in the first launch
        else:
            assert st[3] > 0
            assert {u[:3] for u in units} == set(info["tiles"])    # every destination tile cut into planned bands ...
            assert not any(u[5] for u in units)                   # ... none of them marked
            for t in info["tiles"]:                               # ... that cover its 16 rows once
                rows = sorted((u[3], u[4]) for u in units if u[:3] == t)
                assert rows[0][0] == 0 and rows[-1][1] == sc.TH and all(a[1] == b[0] for a, b in zip(rows, rows[1:])), rows


# ---- 4. flows and data stored in fp16 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("launch", ["first", "second"])
@pytest.mark.parametrize("valid,occ,out_half", [(v, o, h) for v in (False, True) for o in (True, False) for h in (False, True)])
def test_fp16_flow_and_data_are_bit_exact(launch, valid, occ, out_half, dev, native):
    """The sweep frames with the flow and 2 data channels stored in fp16 (ofl_splat_tiled_f16, `_Float16` instantiations): against the
    oracle on their exact fp32 up-conversions, the fp16 result (out_half) as the oracle's fp32 result rounded to fp16."""
    from oracle import oracle
    fr, info, data, ca = sc.make(launch)
    f16 = torch.from_numpy(fr.flow).half()
    assert torch.equal(f16.float(), torch.from_numpy(fr.flow))           # offsets of 1/16, |flow| < 128: exact in fp16
    d16 = torch.from_numpy(np.ascontiguousarray(data[:, :2])).half()
    kw = dict(weight_mask=torch.from_numpy(fr.on).to(dev), occlude=occ, want_valid=valid, out_half=out_half)
    if valid:
        kw["chan_mask_a"] = torch.from_numpy(ca).to(dev)
    dd = d16.float().numpy()
    if valid:
        dd = np.concatenate([dd, ca[:, None].astype(np.float32)], 1)
    ref, _, _ = oracle.apply_s_flow(fr.flow, dd, fr.on, occ, return_density=True)
    exp = ref[:, :2].astype(np.float16) if out_half else ref[:, :2]
    got = []
    for _ in range(2):
        out = native.splat_fwd(f16.to(dev), d16.to(dev), **kw)
        assert "DF16_" in native.last_kernel_name(demangle=False)        # the _Float16 kernels, not an up-converted copy
        got.append((out[0].cpu().numpy(), None if out[1] is None else out[1].cpu().numpy(), native._last_splat_stats.cpu().tolist()))
    for v, m, st in got:
        diff = (_bits(v) != _bits(exp)).any(1)
        assert v.dtype == exp.dtype and not diff.any(), "%d pixels differ; cells by k: %s" % (int(diff.sum()), _by_k(diff, info))
        if valid:
            assert np.array_equal(m, oracle.theta(ref[:, 2]))
        if not VARIANT:
            assert st[0] == 0 and st[1] == 0 and st[2] == 0, st
            assert (st[3] == 0) if launch == "first" else (st[3] > 0), st
    assert _same(got[0][0], got[1][0])


# ---- 3. folds, localised by the library's own redo list ----------------------------------------------------------------------------
def _allowed(units, fr, bands):
    """[n, h, w]: the pixel rows [b0, b1) of the given band units of their tiles."""
    a = np.zeros((fr.n, fr.h, fr.w), bool)
    for b, ty, tx, b0, b1, _ in bands:
        a[b, ty * sc.TH + b0: ty * sc.TH + b1, tx * sc.TW: (tx + 1) * sc.TW] = True
    return a


def _check_fold_bars(r, exp, allowed, what):
    """Outside `allowed` bit for bit; inside values, mask channel and density within the bars; masks exact everywhere."""
    from oracle import oracle
    diff = _differs(r, exp)
    assert not (diff & ~allowed).any(), "%s: %d pixels outside the folded bands differ" % (what, int((diff & ~allowed).sum()))
    np.testing.assert_allclose(r["v"], exp["v"], rtol=RTOL, atol=RTOL * float(np.abs(exp["v"]).max()))
    np.testing.assert_allclose(r["den"], exp["den"], rtol=RTOL, atol=RTOL * float(exp["den"].max()))
    assert np.array_equal(r["warped"], exp["warped"])
    if exp["m"] is not None:
        np.testing.assert_allclose(r["m"], exp["m"], rtol=RTOL, atol=RTOL)
        assert np.array_equal(oracle.theta(r["m"]), oracle.theta(exp["m"]))
    return diff


@pytest.mark.parametrize("c,occ", [(1, True), (2, False), (3, True)])
def test_folds_stay_inside_the_marked_bands(c, occ, dev, native):
    """Cells of 65 and 80 records and a row pair of 2 520 records (splat_cells.fold_frame) in tiles whose bands are planned: the first
    launch marks exactly the bands splat_cells.FOLD_BANDS names, the call counts one fold per marked band, and the pixels that differ
    from the oracle in any bit lie in those bands' rows -- no margin: a band [b0, b1) of a tile reads cell rows b0 .. b1 but phase C
    and the fold path store only its pixel rows b0 .. b1 - 1, and the neighbouring band that shares cell row b1 scans and orders its
    own records.  Elsewhere bit for bit; the marked set is the same in both runs."""
    fr, info, data, ca = sc.make("fold")
    assert sc.record_counts(fr.flow, fr.on, occ) == fr.counts(occ)
    runs = _splat(native, dev, fr, data, ca, c, occ, True)
    exp = _expected(fr, data, ca, c, occ, True)
    marked_runs = []
    for r in runs:
        st, units = r["stats"], _units(native, r, fr)
        assert st[0] == 0 and st[2] == 0, st
        marked = sorted(u for u in units if u[5])
        marked_runs.append(marked)
        if VARIANT:                      # (other switches may cut and fold other bands: the tiles of the redo list bound them)
            allowed = _allowed(units, fr, [(b, ty, tx, 0, sc.TH, 0) for b, ty, tx, _, _, _ in units])
        else:
            assert marked == sorted((b, 0, tx, b0, b1, 1) for b in range(fr.n) for tx, (b0, b1) in sc.FOLD_BANDS.items()), marked
            assert st[1] == len(marked), st
            allowed = _allowed(units, fr, marked)
        diff = _check_fold_bars(r, exp, allowed, "C=%d" % c)
        assert diff.any()                # (the folds do add out of order here: the localisation is tested, not vacuous)
    assert marked_runs[0] == marked_runs[1]


@pytest.mark.parametrize("sigma", [12.0, 16.0, 24.0, 32.0])
def test_rough_flows_fold_only_where_the_library_says(sigma, dev, native):
    """B = 2 1080p flows far rougher than the bench's (sigma 12 ... 32), C = 3 and 2 with the mask channel, hole masks.  A pixel may
    differ from the oracle only in a band the first launch marked, or in one of the four equal bands of a tile that fit but holds a
    cell of more than 64 records (counted here in NumPy): the second launch finds that cell and folds the band.  The call's fold
    count lies between the two."""
    import bench
    from oracle import oracle
    n, h, w = 2, 1080, 1920
    flow = bench.smooth_flow(n, h, w, sigma, 4000 + int(sigma), dev)
    wm = bench.hole_mask(n, h, w, dev)
    ca = bench.hole_mask(n, h, w, dev).flip(1)
    fnp, wmn, can = flow.cpu().numpy(), wm.cpu().numpy(), ca.cpu().numpy()
    shape = types.SimpleNamespace(n=n, h=h, w=w)
    long_cells = [key for key, k in sc.record_counts(fnp, wmn, True).items() if k > sc.LONG]

    def holds_long(u):
        b, ty, tx, b0, b1, _ = u
        return any(lb == b and 0 <= X - tx * sc.TW + 1 <= sc.TW and b0 <= Y - ty * sc.TH + 1 <= b1 for lb, X, Y in long_cells)

    for c in (3, 2):
        g = torch.Generator().manual_seed(77)
        data = torch.rand(n, c, h, w, generator=g) * 100 - 20
        out = native.splat_fwd(flow, data.to(dev), weight_mask=wm, chan_mask_a=ca, want_mask_chan=True, want_density=True, want_warped=True)
        r = dict(v=out[0].cpu().numpy(), m=out[1].cpu().numpy(), den=out[2].cpu().numpy(), warped=out[3].cpu().numpy(),
                 stats=native._last_splat_stats.cpu().tolist(), ws=native._last_splat_ws.cpu().numpy())
        dd = np.concatenate([data.numpy(), can[:, None].astype(np.float32)], 1)
        ref, rwarped, rden = oracle.apply_s_flow(fnp, dd, wmn, True, return_density=True)
        exp = dict(v=ref[:, :c], m=ref[:, c], den=rden, warped=rwarped)
        st, units = r["stats"], _units(native, r, shape)
        assert st[0] == 0 and st[2] == 0, st                          # no image on the two-pass path
        marked = [u for u in units if u[5]]
        found = [u for u in units if not u[5] and holds_long(u)]
        if VARIANT:
            allowed = _allowed(units, shape, [(b, ty, tx, 0, sc.TH, 0) for b, ty, tx, _, _, _ in units])
        else:
            assert len(marked) <= st[1] <= len(marked) + len(found), (st, len(marked), len(found))
            allowed = _allowed(units, shape, marked + found)
        _check_fold_bars(r, exp, allowed, "sigma %g C=%d" % (sigma, c))


# ---- 5. the reference's masked 's' known-answer test (TestApplySFlow.test_masked_s_flow), restated -------------------------------
KAT_H, KAT_W = 480, 512


def _kat_image(nb):
    """A synthetic integer-valued 3-channel image in [0, 255] (the reference reads a photograph; the facts checked do not depend on it)."""
    yy, xx = np.mgrid[0:KAT_H, 0:KAT_W]
    img = np.stack([np.stack([(xx * (7 + b) + yy * 13 + ch * 29 + b * 5) % 256 for ch in range(3)]) for b in range(nb)])
    return img.astype(np.float32)


def _rect(*boxes, fill=False):
    m = np.full((KAT_H, KAT_W), fill)
    for y0, y1, x0, x1 in boxes:
        m[y0:y1, x0:x1] = not fill
    return m


@pytest.mark.parametrize("nb", [1, 3])
def test_masked_s_flow_kat(nb, dev):
    """480 x 512, Flow.from_transforms([['scaling', 256, 240, 1.3]], shape, 's', mask) with the reference's source-mask rectangles and
    zeroed bands; all four combinations of mask / no mask x occlude_zero_flow; the three flow / image pairs with and without
    requires_grad; nb = 3: images of a batch of 3 under the batch-1 flow.  The KAT's image-independent facts -- density masks equal to
    the hand-built rectangles (the single pixel (240, 256) included), pass-through regions equal to the input, the occluding result
    equal to the non-occluding one with the stated rectangle cleared -- and every result bit for bit against the oracle."""
    import oflibpytorch_amd as ofl
    from oracle import oracle
    mask = torch.zeros(1, KAT_H, KAT_W, dtype=torch.bool)
    mask[:, 100:-100, 100:-100] = True
    mask[:, 300:, :250] = False
    mask[:, :300, 250:] = False
    fl = ofl.Flow.from_transforms([['scaling', 256, 240, 1.3]], (KAT_H, KAT_W), 's', mask.to(dev))
    vecs = fl.vecs.clone()
    vecs[:, :, 300:] = 0
    vecs[:, :, :, :100] = 0
    vecs[:, :, :, -100:] = 0
    fmask = fl.mask
    img = torch.from_numpy(_kat_image(nb)).to(dev)
    vn = np.ascontiguousarray(np.broadcast_to(vecs.cpu().numpy(), (nb, 2, KAT_H, KAT_W)))
    mn = np.ascontiguousarray(np.broadcast_to(fmask.cpu().numpy(), (nb, KAT_H, KAT_W)))
    imn = img.cpu().numpy()
    masked_dens = _rect((100 - 42, 300 + 18, 100 - 47, 250 - 2), (300, KAT_H - 100, 250, KAT_W - 100))
    still = _rect((300, KAT_H - 100, 250, KAT_W - 100))                       # masked source region that the flow leaves in place
    moved = _rect((0, 300 + 18, 100 - 47, KAT_W - 100 + 47))                  # everything the unmasked flow moves or covers
    unmasked_occ = moved.copy()
    unmasked_occ[240, 256] = False                                           # the centre of the scaling: a zero vector, occluded
    pairs = [(vecs.clone().requires_grad_(), img), (vecs.clone().requires_grad_(), img.clone().requires_grad_()),
             (vecs, img.clone().requires_grad_())]
    for f, i in pairs:
        got = {}
        for masked in (True, False):
            for occ in (False, True):
                out, dens = ofl.apply_s_flow(f, i, fmask if masked else None, occlude_zero_flow=occ)
                assert out.grad_fn is not None
                o, d = out.detach().cpu().numpy(), dens.cpu().numpy()
                ref, rwarped = oracle.apply_s_flow(vn, imn, mn if masked else None, occ)
                assert _same(o, ref), "masked=%s occlude=%s: values differ from the oracle" % (masked, occ)
                assert np.array_equal(d, rwarped)
                got[(masked, occ)] = (o, d)
        o, d = got[(True, False)]
        assert (d == masked_dens).all()
        assert np.array_equal(o[:, :, still], imn[:, :, still])
        o2, d2 = got[(True, True)]
        assert _same(o2, o)
        assert (d2 == (masked_dens & ~still)).all()
        o3, d3 = got[(False, False)]
        assert d3.all()
        assert np.array_equal(o3[:, :, ~moved], imn[:, :, ~moved])
        o4, d4 = got[(False, True)]
        assert (d4 == unmasked_occ).all()
        assert np.array_equal(o4[:, :, ~unmasked_occ], imn[:, :, ~unmasked_occ])
