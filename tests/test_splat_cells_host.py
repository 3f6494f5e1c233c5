"""CPU tier: the frames of tests/splat_cells.py do what tests/test_gpu_splat_cells.py relies on -- exactly the intended records per
cell, tiles that fit or overflow the gather kernel's LDS as stated, subtiles whose end points stay in one destination tile, flows
exact in fp16, records that arrive out of raster order by construction, and data whose class sums change with the order of their
additions (the evidence that a misordering would show)."""
import numpy as np
import pytest

import splat_cells as sc

KINDS = ("first", "second", "fold")
ORDER_FRACTION = {"fp32": 0.97, "fp16": 0.90}   # share of the cells of k >= 3 whose class sums change in some order (measured 99 % / 94 %)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("occlude", [False, True])
def test_records_per_cell_are_exactly_the_intended(kind, occlude):
    """The splat's records per cell, counted independently in NumPy (end points, weight mask, zero-vector rule), are the constructor's
    counts; occlude_zero_flow removes exactly the zero-vector source of the cells that hold one."""
    fr, info, _, _ = sc.make(kind)
    got = sc.record_counts(fr.flow, fr.on, occlude)
    assert got == fr.counts(occlude)
    for key, k in info["k_of"].items():
        if k is not None:
            kk, zero = fr.cells[key]
            assert kk == k and got.get(key, 0) == k - (1 if (occlude and zero) else 0)
    zeros = [key for key, (_, z) in fr.cells.items() if z]
    assert len(zeros) >= 4 * fr.n                                        # exactly-zero vectors among the sources of several k
    for b, X, Y in zeros:
        assert fr.on[b, Y, X] and not fr.flow[b, :, Y, X].any()


def test_tile_loads():
    """'first': every destination tile fits the LDS of the 3-channel kernel (1 792 records); 'second': every one holds more than the
    1-2 channel kernel's 2 048; 'fold': columns 0-2 over 2 048 (column 2 in one row pair), column 3 fits.  All records of a frame
    land in its destination tiles, and every k of the sweep is in every destination tile."""
    for kind, lo, hi in (("first", 1, 1792), ("second", 2049, 1 << 30)):
        fr, info, _, _ = sc.make(kind)
        loads = sc.tile_records(fr.counts(False))
        assert set(loads) == set(info["tiles"])
        assert all(lo <= v <= hi for v in loads.values()), loads
        for b, _, tx in info["tiles"]:
            ks = {k for (bb, X, _), k in info["k_of"].items() if bb == b and X // sc.TW == tx}
            assert set(sc.K_SWEEP) <= ks
    fr, info, _, _ = sc.make("fold")
    cnt = fr.counts(False)
    loads = sc.tile_records(cnt)
    for b in range(fr.n):
        assert min(loads[(b, 0, 0)], loads[(b, 0, 1)], loads[(b, 0, 2)]) > 2048 and loads[(b, 0, 3)] <= 1792
        pair = sum(k for (bb, X, Y), k in cnt.items() if bb == b and X // sc.TW == 2 and Y in (8, 9))
        assert pair > 2048
        assert cnt[(b, 10, 4)] == 65 and cnt[(b, sc.TW + 20, 10)] == 80
        assert max(k for (bb, X, Y), k in cnt.items() if bb == b and (X, Y) not in ((10, 4), (sc.TW + 20, 10))) <= sc.LONG


@pytest.mark.parametrize("kind", KINDS)
def test_subtiles_stay_in_one_destination_tile(kind):
    """The destination pixels a subtile's end points touch lie in one tile (its list entry goes to one tile only), except the one
    subtile of the cross-tile hole, which both tile columns 0 and 1 of image 0 scan; no tile lists more than a quarter of kBinCap."""
    fr, info, _, _ = sc.make(kind)
    tiles = {}
    for b, sy, sx in np.argwhere(fr.on):
        X = int(np.floor(fr.flow[b, 0, sy, sx] + sx))
        Y = int(np.floor(fr.flow[b, 1, sy, sx] + sy))
        tt = {(X // sc.TW, Y // sc.TH), ((X + 1) // sc.TW, (Y + 1) // sc.TH)}
        tiles.setdefault((int(b), int(sy) // sc.SUBH, int(sx) // sc.SUBW), set()).update(tt)
    multi = {s: t for s, t in tiles.items() if len(t) > 1}
    if info["cross"] is not None:
        b, sx, sy = info["cross"]
        assert multi == {(b, sy // sc.SUBH, sx // sc.SUBW): {(0, 0), (1, 0)}}
    else:
        assert multi == {}
    per_tile = {}
    for (b, _, _), t in tiles.items():
        for tt in t:
            per_tile[(b,) + tt] = per_tile.get((b,) + tt, 0) + 1
    assert max(per_tile.values()) <= 512 // 4


@pytest.mark.parametrize("kind", KINDS)
def test_flows_are_exact_in_fp16(kind):
    fr, _, data, _ = sc.make(kind)
    assert np.abs(fr.flow).max() < 128
    assert np.array_equal(fr.flow.astype(np.float16).astype(np.float32), fr.flow)
    h = data.astype(np.float16)
    assert np.isfinite(h).all() and (np.abs(h) >= np.float16(2.0 ** -14)).all()   # the data's exponents fit fp16's normal range


@pytest.mark.parametrize("kind", ["first", "second"])
def test_records_arrive_out_of_raster_order(kind):
    """Every sweep cell takes its records (beside an exactly-zero source in the destination row) from two subtiles, and from k = 3 on
    from a horizontally adjacent pair of pixels of different lanes, so the scan's insertion order (pixel j of every lane before pixel
    j + 1, subtile by subtile) is not raster order."""
    fr, info, _, _ = sc.make(kind)
    cross = None if info["cross"] is None else info["cross"][1:]
    checked = 0
    for key, k in info["k_of"].items():
        recs = [p for p in fr.records(key) if p != (key[1], key[2])]
        if k is None or cross in recs:
            continue                                                     # (medium cells; the cross-tile cell is built by hand)
        subs = {(y // sc.SUBH, x // sc.SUBW) for x, y in recs}
        pairs = {(x, y) for x, y in recs if (x + 1, y) in set(recs) and (x + 1) % 4 == 0}
        if len(recs) >= 2:
            assert len(subs) >= 2, (key, k, recs)
        if len(recs) >= 3:
            assert pairs and sc.interleaved(recs) != recs, (key, k, recs)
            checked += 1
    assert checked >= 13 * len(info["tiles"])


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_class_sums_depend_on_the_order(prec):
    """For the sweep cells of k >= 3, the fp32 class sums (4 corner classes x 3 channels) added in reversed or in the scan's
    interleaved order differ in at least one bit from the raster-order sums in at least ORDER_FRACTION of the cells -- every cell of
    k >= 6 included.  With the data rounded to fp16 first (the fp16 tests' data) the products are exact and only the additions round;
    the share is smaller, still a large majority."""
    fr, info, data, _ = sc.make("first")
    d = data[:, :3] if prec == "fp32" else data[:, :3].astype(np.float16).astype(np.float32)
    tot = hit = 0
    for key, k in info["k_of"].items():
        if k is None or fr.cells[key][0] < 3:
            continue
        recs = fr.records(key)
        ref = sc.class_sums(fr, key, d, recs).view(np.uint32)
        differs = any(not np.array_equal(sc.class_sums(fr, key, d, o).view(np.uint32), ref) for o in (recs[::-1], sc.interleaved(recs)))
        tot += 1
        hit += differs
        if k >= 6:
            assert differs, (key, k)
    assert tot >= 15 * 4 * 8 and hit >= ORDER_FRACTION[prec] * tot, (hit, tot)


def test_mechanism_table():
    """DESIGN.md 3.2's rows, per channel count: the thresholds the sweep straddles."""
    rows = lambda nc: [sc.mechanism(k, nc) for k in (1, 2, 3, 4, 5, 6, 7, 8, 9, 64, 65)]
    assert rows(3) == ["none", "none", "network5", "network5", "lane-network", "lane-network", "wave", "wave", "wave", "wave", "fold"]
    assert rows(2) == rows(1) == ["none", "none", "network5", "network5"] + ["lane-network"] * 4 + ["wave", "wave", "fold"]


def test_redo_units_decode():
    """The workspace layout the decoder assumes (ofl_kernels.hip, splat_pass_words), on a synthetic workspace."""
    n, h, w, cap = 2, 40, 130, 512
    tx_n, ty_n = 3, 3
    tiles = n * tx_n * ty_n
    off = 8 + 4 + 20 + cap * tiles
    ws = np.zeros(off + 2 * 16 * tiles, np.int32)
    entries = [((1 * 9 + 2 * 3 + 1), 0 | 6 << 8), ((0 * 9 + 0 * 3 + 2), 4 | 6 << 8 | 1 << 16)]
    ws[6] = len(entries)
    for i, (t, v) in enumerate(entries):
        ws[off + 2 * i], ws[off + 2 * i + 1] = t, v
    assert sc.redo_units(ws, n, h, w, cap) == [(1, 2, 1, 0, 6, 0), (0, 0, 2, 4, 6, 1)]
