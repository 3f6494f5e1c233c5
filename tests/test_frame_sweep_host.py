"""CPU tier of the frame sweep (tests/frame_sweep.py): the inputs and the reach table that keep the GPU tier from passing vacuously,
checked on the oracle and on the recorded table alone -- no GPU, no library."""
import numpy as np
import pytest

import frame_sweep as fs
import splat_cells as sc
import test_gpu_warp_kernel_choice as kc


def test_the_frame_lines():
    assert len(fs.WIDTHS) == 48 and len(fs.HEIGHTS) == 37 and len(fs.FRAMES) == 2 * 48 + 2 * 37 - 4      # (17 and 66 x 35 and 36 are on both lines)
    assert min(min(f) for f in fs.FRAMES) == 2
    # both W = 1 (mod 32) and H = 1 (mod 64) -- and the one-row last column group, the two-pixel last tile over a ragged last row
    assert (65, 35) in fs.FRAMES and (129, 35) in fs.FRAMES and (66, 33) in fs.FRAMES and (66, 65) in fs.FRAMES and (17, 34) in fs.FRAMES
    assert {w % 64 for w in fs.WIDTHS} >= {0, 1, 2, 63} and {h % 64 for h in fs.HEIGHTS} >= {0, 1, 2, 3, 62, 63}
    assert {h % 16 for h in fs.HEIGHTS} >= {0, 1, 2, 3, 14, 15}


@pytest.mark.parametrize("line", ["width", "height"])
def test_samples_leave_over_every_border_and_land_on_the_named_positions(line):
    for h, w in (fs.WIDTH_LINE if line == "width" else fs.HEIGHT_LINE):
        t = fs.content(h, w)
        sx, sy = fs.sample_positions(t["flow"])
        if min(h, w) >= 8:
            out = dict(left=(sx < 0), right=(sx > w - 1), top=(sy < 0), bottom=(sy > h - 1))
            for side, where in out.items():
                assert where.any(), "%d x %d: no sample leaves across the %s border" % (h, w, side)
                assert where.reshape(fs.IMAGES, -1).any(1).sum() >= 2, (h, w, side)
        for y, x in t["named"]["integer"]:
            assert (sx[:, y, x] == np.floor(sx[:, y, x])).all() and (sy[:, y, x] == np.floor(sy[:, y, x])).all(), (h, w, y, x)
        assert t["named"]["integer"] and t["named"]["zero"]
        for y, x in t["named"]["last_row"]:
            assert (sy[:, y, x] == h - 1).all(), (h, w, y, x)
        for y, x in t["named"]["last_col"]:
            assert (sx[:, y, x] == w - 1).all(), (h, w, y, x)
        assert t["named"]["last_row"] and t["named"]["last_col"]
        amp = np.abs(t["flow"]).max()
        assert amp < 140, (h, w, amp)


@pytest.mark.parametrize("line", ["width", "height"])
def test_valid_area_has_both_values_and_keeps_a_quarter(line):
    from oracle import oracle
    for h, w in (fs.WIDTH_LINE if line == "width" else fs.HEIGHT_LINE):
        t = fs.content(h, w)
        valid = oracle.theta(oracle.G(t["flow"], t["m1"][:, None].astype(np.float32))[:, 0]) & t["m2"]
        for b in range(fs.IMAGES):
            assert valid[b].any() and not valid[b].all(), (h, w, b)
            assert valid[b].mean() >= 0.25, "%d x %d image %d: %.3f of the frame valid" % (h, w, b, valid[b].mean())
        assert not t["m1"].all() and not t["m2"].all()


def test_the_four_images_differ_in_every_plane():
    for h, w in fs.FRAMES:
        t = fs.content(h, w)
        for key in ("flow", "src", "other", "m1", "m2"):
            a = t[key] if t[key].ndim == 4 else t[key][:, None]
            for i in range(fs.IMAGES):
                for j in range(i + 1, fs.IMAGES):
                    for plane in range(a.shape[1]):
                        assert not np.array_equal(a[i, plane], a[j, plane]), (h, w, key, i, j, plane)


def _longest_cell(flow, on, sign):
    """The largest number of records in one cell, as splat_cells.record_counts counts them (end point in fp32, the weight mask, the
    zero-vector rule, cells clamped to [-2, W] x [-2, H]) without its dict."""
    f = flow * np.float32(sign)
    n, _, h, w = f.shape
    x = f[:, 0] + np.arange(w, dtype=np.float32)[None, None, :]
    y = f[:, 1] + np.arange(h, dtype=np.float32)[None, :, None]
    act = on & ~((np.abs(f[:, 0]) < 1e-3) & (np.abs(f[:, 1]) < 1e-3))
    X, Y = np.clip(np.floor(x), -2, w).astype(np.int64) + 2, np.clip(np.floor(y), -2, h).astype(np.int64) + 2
    key = (np.arange(n)[:, None, None] * (h + 3) + Y) * (w + 3) + X
    return int(np.bincount(key[act]).max())


def test_splat_inputs_keep_every_cell_at_or_under_64_records():
    """The gather splat sums a cell of up to 64 records in order (tests/splat_cells.py): the sweep's flows, as 's' flows with and
    without the weight mask and with the sign of splat_sum, stay under that in every frame the splat sweep runs."""
    t = fs.content(17, 36)
    assert _longest_cell(t["flow"], t["m1"], 1.0) == max(sc.record_counts(t["flow"], t["m1"], True).values())
    for h, w in fs.FRAMES:
        if w < 4:
            continue
        t = fs.content(h, w)
        for mask in (np.ones_like(t["m1"]), t["m1"]):
            for sign in (1.0, -1.0):                                       # (-1: splat_sum, the transpose of the warp)
                assert _longest_cell(t["flow"], mask, sign) <= 64, (h, w, sign)


def test_the_vectorised_splat_sum_restatement_equals_the_loops():
    """tests/test_gpu_frame_sweep_splat.py holds splat_sum to special_values.splat_sum_restated; here that equals the loop restatement
    of tests/test_gpu_parity.py bit for bit on three small swept frames (the loops take seconds on a large one)."""
    import special_values as sv
    import test_gpu_parity as tp
    for h, w in ((2, 35), (5, 36), (17, 9)):
        t = fs.content(h, w)
        data = np.ascontiguousarray(t["src"][:2, :2] - np.float32(100))
        got, want = sv.splat_sum_restated(t["flow"][:2], data), tp._splat_sum_reference(t["flow"][:2], data, -1.0, 1.0)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.abs(want).max() > 10, (h, w)


def _signature(case):
    c = case["c"] if case["c"] <= 3 else (case["c"] - 1) % 3 + 1 if fs.choose(**_opts(case))[0] not in ("chan", "chan_rows") else 0
    valid = bool(case.get("valid")) and (case["c"] <= 3 or c == 0)
    return (case["kind"], c, valid, case.get("addend"), bool(case.get("src_b")), bool(case.get("dst_flags")), bool(case.get("flags")),
            bool(case.get("to_u8")))


def _opts(case):
    return {k: v for k, v in case.items() if k != "id"}


def test_the_restated_choice_agrees_with_the_recorded_table():
    """Every recorded case: launches with the same restated choice and the same options have ONE recorded kernel name, and a kernel
    name has one restated (family, tiles per block)."""
    names, kernels = {}, {}
    for case in kc.CASES:
        choice = fs.choose(**_opts(case))
        assert choice[0] not in ("generic", "split"), case["id"]
        names.setdefault((choice, _signature(case)), set()).add(kc.RECORDED[case["id"]])
        kernels.setdefault(kc.RECORDED[case["id"]], set()).add(choice[:2])
    assert all(len(v) == 1 for v in names.values()), [(k, sorted(v)) for k, v in names.items() if len(v) > 1][:3]
    assert all(len(v) == 1 for v in kernels.values()), [(k, sorted(v)) for k, v in kernels.items() if len(v) > 1][:3]
    for name, fam in kernels.items():
        family, t = next(iter(fam))
        tag = {"rows": "warp_bwd_rows_kernel", "column": "warp_bwd_lds_column_kernel", "pair": "warp_bwd_lds_kernel",
               "chan": "warp_bwd_lds_chan_kernel", "chan_rows": "warp_bwd_lds_chan_kernel"}[family]
        assert tag in name and (family not in ("rows", "column") or ("<%d," % t) in name or ("ILi%dE" % t) in name), (name, fam)


def test_every_recorded_kernel_meets_the_residue_condition():
    """The reach table: for each recorded kernel (and each entry of the 16-bit table) the frames it can be put on, from the thresholds;
    on them residues 0, 1 and T - 1 of its tile width and column height, and W % 4 = 1, 2, 3 where the launcher gives it such widths
    (frame_sweep.residue_gaps states the W % 4 == 0 analogue).  Printed with -s."""
    rows = fs.recorded_cases() + [(str(key), case) for key, case in fs.x16_cases()]
    assert len(fs.recorded_cases()) == len({(c["kind"], kc.RECORDED[c["id"]]) for c in kc.CASES}) == 121 and len(fs.x16_cases()) == 39
    lacking = {}
    for name, case in rows:
        frames = fs.frames_for(case)
        tw, th = fs.tile_of(case)
        print("%3d frames, tile %2d x %2d, up to %8d pixels  %-52s %s" % (len(frames), tw, th, max(h * w * n for h, w, n in frames),
                                                                           case.get("id", "x16"), name))
        assert all(fs.choose(**dict(_opts(case), h=h, w=w, n=n)) == fs.choose(**_opts(case)) for h, w, n in frames)
        assert max(h * w * n for h, w, n in frames) <= 15e6
        gaps = fs.residue_gaps(case, frames)
        if gaps:
            lacking[case.get("id", name)] = gaps
    assert not lacking, lacking
    # the class the thresholds rule out is ruled out here too: the pair kernel of a plain launch needs g1 >= kColumnMinGroups > g4
    pair = next(case for key, case in fs.x16_cases() if key == ("pair", 2, 1, False))
    reached = {(h, w) for h, w, _ in fs.frames_for(pair)}
    assert fs.choose(**pair)[0] == "pair" and reached == {(h, w) for h, w in fs.FRAMES if h > 16 and w % 4 and w >= 4}
