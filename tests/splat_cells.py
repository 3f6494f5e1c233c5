"""Host side of tests/test_gpu_splat_cells.py: frames in which chosen destination cells of the forward splat receive EXACTLY k
records, with data whose class sums depend on the order they are added in.

A *cell* is the unit square [X, X + 1) x [Y, Y + 1) that a source end point falls in; the gather splat keeps one
chain of records per cell and must add a cell's records in raster order of their source pixels, the order of the reference's
scatter_add_.  It puts them in that order by a different mechanism for each cell length (`mechanism`), so a sweep over k reaches
every one of them.

Layout of a frame built here: every 64-wide column of tiles holds one DESTINATION tile (tile row 0; its cells lie at even offsets
from the tile origin, X - dx0 in 0, 2 .. 62 and Y - dy0 in 0, 2 .. 14, so that no destination pixel is served by two cells and no
cell touches a neighbouring tile) above 2 or 3 tile rows of SOURCES for it.  The source rows are two streams of 16 x 2 subtiles (the
bin kernel's unit: 8 lanes of 4 horizontally adjacent pixels); a cell of k >= 2 takes the first half of its records from one stream
and the rest from the other, each part a horizontal run that straddles a lane boundary.  The scan inserts pixel j of every lane of
a wave before pixel j + 1, and subtiles arrive in the order of the tile's list, so the chains come out of raster order.  Source
pixels that belong to no cell are switched off by the weight mask.  Sub-cell offsets are distinct multiples of 1/16 and every
|flow| < 128, so the same flow is exact in fp16.
"""
import numpy as np

TW, TH = 64, 16          # destination tile of the gather splat (the library reports it: _native.splat_tile_geometry())
SUBW, SUBH = 16, 2       # source subtile: 8 lanes of 4 horizontally adjacent pixels
LONG = 64                # longest cell the gather splat sums in order (kSpLong)
K_SWEEP = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 31, 32, 33, 63, 64)
ZERO_K = (1, 4, 7, 13, 33, 63)   # with one copy of the sweep: the cells that hold an exactly-zero source
_OFFS = np.array([(ox, oy) for oy in range(1, 16) for ox in range(1, 16)], np.int64)   # 225 distinct sub-cell offsets (1/16 units)


def net_size(nc):
    """Longest cell one lane's sorting network orders: 6 records with 3 data channels, 8 with 1-2 (SpLay::kNet)."""
    return 6 if nc >= 3 else 8


def mechanism(k, nc):
    """The row of DESIGN.md 3.2's phase S that a cell of k records reaches (nc: data channels of the channel group, 1-3)."""
    if k <= 2:
        return "none"            # a + b from +0 commutes: phase S skips the cell
    if k <= 4:
        return "network5"        # 5-comparator network, chain re-linked
    if k <= net_size(nc):
        return "lane-network"    # sorting network in one lane's registers, class sums written over part A
    if k <= LONG:
        return "wave"            # sp2_order_big_cell (first launch) / sp2_big_cells_block (second launch)
    return "fold"                # the band is marked and summed with LDS float atomics


def order_data(shape, rng):
    """A random sign times 2**e, e uniform in [-12, 12], with a random 23-bit mantissa: sums of a few such terms depend on their order."""
    e = rng.integers(-12, 13, size=shape)
    man = 1.0 + rng.integers(0, 1 << 23, size=shape) / float(1 << 23)
    sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    return (sign * man * np.exp2(e)).astype(np.float32)


class _Stream:
    """Source pixels of a run of subtiles, handed out in raster order within each subtile (row 0 left to right, then row 1)."""

    def __init__(self, subtiles):
        self.subs, self.i, self.j = list(subtiles), 0, 0

    def _advance(self, m):
        self.j += m
        while self.j >= SUBW * SUBH:
            self.i, self.j = self.i + 1, self.j - SUBW * SUBH

    def take(self, m, straddle=False):
        """m pixels of a run in raster order; `straddle` (m >= 2): start it where its first step from one lane (4 pixels) to the next
        stays inside a subtile row, i.e. joins two horizontally adjacent pixels."""
        if straddle and m >= 2:
            ok = (lambda s: s <= SUBW - 5) if m >= 5 else (lambda s: s % 4 > 4 - m and s + m <= SUBW)
            col = self.j % SUBW
            start = next((s for s in range(col, SUBW) if ok(s)), None)
            if start is None:                                                # (not in this subtile row: the next one)
                start = SUBW + next(s for s in range(SUBW) if ok(s))
            self._advance(start - col)
        out = []
        for _ in range(m):
            if self.i >= len(self.subs):
                raise ValueError("source pool exhausted")
            sx0, sy0 = self.subs[self.i]
            out.append((sx0 + self.j % SUBW, sy0 + self.j // SUBW))
            self._advance(1)
        return out

    def left(self):
        return (len(self.subs) - self.i) * SUBW * SUBH - self.j


class CellFrame:
    """A flow, weight mask and per-cell record counts, built cell by cell."""

    def __init__(self, n, h, w, seed):
        self.n, self.h, self.w = n, h, w
        self.flow = np.zeros((n, 2, h, w), np.float32)
        self.on = np.zeros((n, h, w), bool)                      # the weight mask
        self.rng = np.random.default_rng(seed)
        self.cells = {}                                          # (b, X, Y) -> (records with occlude_zero_flow off, has an exactly-zero source)
        self.sources = {}                                        # (b, X, Y) -> [(sx, sy), ...]

    def add_cell(self, b, X, Y, sources, zero=False):
        """The cell (X, Y) of image b receives one record from every source pixel, plus (zero) one from the pixel (X, Y) itself with
        an exactly-zero vector (a record only while occlude_zero_flow is off)."""
        assert 0 <= X < self.w - 1 and 0 <= Y < self.h - 1 and (b, X, Y) not in self.cells
        offs = _OFFS[self.rng.choice(len(_OFFS), size=len(sources), replace=False)]
        for (sx, sy), (ox, oy) in zip(sources, offs):
            assert not self.on[b, sy, sx], "source pixel used twice"
            fx, fy = X + ox / 16.0 - sx, Y + oy / 16.0 - sy
            assert abs(fx) < 128 and abs(fy) < 128
            self.flow[b, 0, sy, sx], self.flow[b, 1, sy, sx] = fx, fy
            self.on[b, sy, sx] = True
        srcs = list(sources)
        if zero:
            assert not self.on[b, Y, X]
            self.on[b, Y, X] = True                             # (its flow stays 0: the end point is (X, Y) itself)
            srcs.append((X, Y))
        self.cells[(b, X, Y)] = (len(srcs), bool(zero))
        self.sources[(b, X, Y)] = srcs

    def counts(self, occlude):
        """Intended records per cell: occlude_zero_flow drops the exactly-zero source (a cell left with none is not listed)."""
        out = {}
        for key, (k, z) in self.cells.items():
            kk = k - (1 if (occlude and z) else 0)
            if kk:
                out[key] = kk
        return out

    def records(self, key, occlude=False):
        """Source pixels of a cell's records, in raster order."""
        k, z = self.cells[key]
        srcs = self.sources[key][:k - 1] if (occlude and z) else self.sources[key]
        return sorted(srcs, key=lambda p: (p[1], p[0]))


def record_counts(flow, on, occlude, flow_sign=1.0):
    """Records per cell as the splat forms them, counted independently in NumPy: end point s * flow + (x, y) in fp32, the weight
    mask, the zero-vector rule (both components strictly inside (-1e-3, 1e-3)), the cell (floor x, floor y) clamped to [-2, W] x
    [-2, H] as the kernels clamp it.  -> {(b, X, Y): count}."""
    flow = np.asarray(flow, np.float32) * np.float32(flow_sign)
    n, _, h, w = flow.shape
    x = flow[:, 0] + np.arange(w, dtype=np.float32)[None, None, :]
    y = flow[:, 1] + np.arange(h, dtype=np.float32)[None, :, None]
    act = np.broadcast_to(np.asarray(on, bool), (n, h, w)).copy()
    if occlude:
        act &= ~((np.abs(flow[:, 0]) < 1e-3) & (np.abs(flow[:, 1]) < 1e-3))
    X = np.clip(np.floor(x), -2, w).astype(np.int64)
    Y = np.clip(np.floor(y), -2, h).astype(np.int64)
    b = np.broadcast_to(np.arange(n)[:, None, None], (n, h, w))
    keys = np.stack([b[act], X[act], Y[act]], 1)
    if not len(keys):
        return {}
    uk, cnt = np.unique(keys, axis=0, return_counts=True)
    return {(int(a), int(c), int(d)): int(k) for (a, c, d), k in zip(uk, cnt)}


def interleaved(recs):
    """A cell's records in the scan's insertion order: subtile by subtile, and inside a subtile pixel j of every lane before pixel
    j + 1 (the lanes of a subtile row by row)."""
    return sorted(recs, key=lambda p: (p[1] // SUBH, p[0] // SUBW, p[0] % 4, p[1] % SUBH, (p[0] % SUBW) // 4))


def class_sums(frame, key, data, recs):
    """fp32 corner-class sums of one cell (4 classes x channels), its records added in the order of `recs`.  Weights and products
    round as phase C forms them: (1 - fy) * (1 - fx) etc., then w * d, then the add."""
    b = key[0]
    c = data.shape[1]
    acc = np.zeros((4, c), np.float32)
    one = np.float32(1.0)
    for sx, sy in recs:
        ex = np.float32(frame.flow[b, 0, sy, sx]) + np.float32(sx)
        ey = np.float32(frame.flow[b, 1, sy, sx]) + np.float32(sy)
        fx, fy = np.float32(ex - np.floor(ex)), np.float32(ey - np.floor(ey))
        wx0, wy0 = np.float32(one - fx), np.float32(one - fy)
        wv = (np.float32(wy0 * wx0), np.float32(wy0 * fx), np.float32(fy * wx0), np.float32(fy * fx))
        for ci in range(4):
            for ch in range(c):
                acc[ci, ch] = np.float32(acc[ci, ch] + np.float32(wv[ci] * data[b, ch, sy, sx]))
    return acc


def _pools(tiles_x, src_rows):
    half = src_rows * TH // 2                                          # rows per stream (even)
    pools = []
    for tx in range(tiles_x):
        subs = [[(tx * TW + sx, sy) for sy in range(r0, r0 + half, SUBH) for sx in range(0, TW, SUBW)] for r0 in (TH, TH + half)]
        pools.append((_Stream(subs[0]), _Stream(subs[1])))
    return pools


def _slots(tx, rng):
    """The cell positions of destination tile column tx (even offsets), in a random order: pop() hands them out."""
    dx0 = tx * TW
    slots = [(dx0 + 2 * i, 2 * j) for j in range(TH // 2) for i in range(TW // 2)]
    return [slots[i] for i in rng.permutation(len(slots))]


def _sweep_cell(fr, b, X, Y, k, zero, A, B):
    kk = k - (1 if zero else 0)                                        # (the zero-vector source is one of the k)
    a = (kk + 1) // 2
    srcs = (A.take(a, straddle=True) if a else []) + (B.take(kk - a, straddle=True) if kk - a else [])
    fr.add_cell(b, X, Y, srcs, zero=zero)


def _fill(fr, b, slots, A, B, rng, info, lo=5, hi=12):
    """Medium cells of lo .. hi records in the remaining slots, while the pools last."""
    while slots:
        k = int(rng.integers(lo, hi + 1))
        a = (k + 1) // 2
        if A.left() < a or B.left() < k - a:
            break
        X, Y = slots.pop()
        fr.add_cell(b, X, Y, A.take(a) + B.take(k - a))
        info["k_of"][(b, X, Y)] = None


def sweep_frame(n=2, tiles_x=4, overflow=False, seed=0):
    """The k sweep in one frame.  overflow=False: every destination tile holds 4 cells of every k in K_SWEEP (copy 1 with an
    exactly-zero source among its k), about 1 240 records: it fits the gather kernel's LDS (1 792 records with 3 data channels,
    2 048 with 1-2).  overflow=True: one copy of the sweep (the ZERO_K cells with a zero source) plus medium cells of 5 ... 12
    records, about 2 300 per tile: every destination tile is cut into bands in the first launch and the same k are ordered in the
    second.  Image 0 also sends one source pixel of tile column 0's pool to a 3-record cell of tile column 1 (a subtile scanned by
    both tiles: `info['cross']`).
    Returns (frame, info): info = {'tiles': destination tiles (b, ty, tx), 'k_of': {(b, X, Y): k of the sweep, None for a medium
    cell}, 'cross': (b, sx, sy)}."""
    src_rows = 3 if overflow else 2
    copies = 1 if overflow else 4
    fr = CellFrame(n, TH * (1 + src_rows), TW * tiles_x, seed)
    rng = np.random.default_rng(seed + 1)
    info = {"tiles": [], "k_of": {}, "cross": None}
    for b in range(n):
        pools = _pools(tiles_x, src_rows)
        cross_px = None
        if b == 0 and tiles_x >= 2:
            cross_px = pools[0][0].take(1)[0]                          # (tile column 0's pool: its subtile is listed for both tiles)
            info["cross"] = (b, cross_px[0], cross_px[1])
        for tx in range(tiles_x):
            A, B = pools[tx]
            slots = _slots(tx, rng)
            info["tiles"].append((b, 0, tx))
            for cp in range(copies):
                for k in K_SWEEP:
                    X, Y = slots.pop()
                    zero = (cp == 1) if copies > 1 else (k in ZERO_K)
                    _sweep_cell(fr, b, X, Y, k, zero, A, B)
                    info["k_of"][(b, X, Y)] = k
            if cross_px is not None and tx == 1:
                X, Y = slots.pop()
                fr.add_cell(b, X, Y, [cross_px] + A.take(1) + B.take(1))
                info["k_of"][(b, X, Y)] = 3
            if overflow:
                _fill(fr, b, slots, A, B, rng, info)
    return fr, info


FOLD_BANDS = {0: (4, 6), 1: (10, 12), 2: (9, 10)}   # tile column -> the band of pixel rows [b0, b1) that fold_frame's tiles mark


def fold_frame(n=2, seed=0):
    """Tiles whose bands the first launch MARKS (summed with LDS float atomics, to a tolerance), beside tiles that stay exact.  Tile
    column 0: a cell of 65 records at Y = 4; column 1: a cell of 80 at Y = 10 -- both in tiles pushed over the LDS capacity by medium
    cells, so that the bands are planned and the pixel rows the long cell serves (4-5, 10-11) are marked.  Column 2: 32 cells of 40
    records at Y = 8 and 31 at Y = 9, a row pair of 2 520 records, more than the LDS holds whatever the band: pixel row 9, which both
    rows serve, is marked.  Column 3: one copy of the k sweep in a tile that fits.  Returns (frame, info) as sweep_frame."""
    fr = CellFrame(n, TH * 4, TW * 4, seed)
    rng = np.random.default_rng(seed + 1)
    info = {"tiles": [], "k_of": {}, "cross": None}
    for b in range(n):
        pools = _pools(4, 3)
        for tx in range(4):
            A, B = pools[tx]
            dx0 = tx * TW
            info["tiles"].append((b, 0, tx))
            slots = _slots(tx, rng)
            if tx in (0, 1):
                X, Y, k = (dx0 + 10, 4, 65) if tx == 0 else (dx0 + 20, 10, 80)
                slots.remove((X, Y))
                _sweep_cell(fr, b, X, Y, k, False, A, B)
                info["k_of"][(b, X, Y)] = k
                _fill(fr, b, slots, A, B, rng, info)
            elif tx == 2:
                for i in range(32):
                    for X, Y in ((dx0 + 2 * i, 8), (dx0 + 2 * i + 1, 9)):
                        if X - dx0 <= 62:
                            fr.add_cell(b, X, Y, A.take(20) + B.take(20))
                            info["k_of"][(b, X, Y)] = 40
            else:
                for k in K_SWEEP:
                    X, Y = slots.pop()
                    _sweep_cell(fr, b, X, Y, k, k in ZERO_K, A, B)
                    info["k_of"][(b, X, Y)] = k
    return fr, info


def hole_mask(frame, info, tiles_with_holes, frac=0.12, seed=5):
    """The mask channel: False on a fraction of the sources of the listed destination tiles (b, tx), and on the cross pixel; True
    elsewhere -- the tiles in between keep phase C's all-valid shortcut."""
    rng = np.random.default_rng(seed)
    m = np.ones((frame.n, frame.h, frame.w), bool)
    for (b, X, Y), srcs in sorted(frame.sources.items()):
        if (b, X // TW) in tiles_with_holes:
            for sx, sy in srcs:
                if rng.random() < frac:
                    m[b, sy, sx] = False
    if info.get("cross") is not None:
        b, sx, sy = info["cross"]
        m[b, sy, sx] = False
    return m


_MADE = {}


def make(kind):
    """The frames both test files use (cached): 'first' (the sweep in tiles that fit), 'second' (in tiles that overflow) or 'fold'.
    -> (frame, info, data [n, 5, h, w] fp32 of order_data, mask channel [n, h, w] bool)."""
    if kind not in _MADE:
        if kind == "fold":
            fr, info = fold_frame(seed=21)
            holes = {(1, 0), (1, 2)}
        else:
            fr, info = sweep_frame(overflow=(kind == "second"), seed=3 if kind == "first" else 13)
            holes = {(0, 2), (1, 1), (1, 3)}
        data = order_data((fr.n, 5, fr.h, fr.w), np.random.default_rng(77))
        _MADE[kind] = (fr, info, data, hole_mask(fr, info, holes))
    return _MADE[kind]


def tile_records(counts):
    """Records per destination tile (b, ty, tx) of a {(b, X, Y): k} map whose cells each lie inside one tile."""
    out = {}
    for (b, X, Y), k in counts.items():
        key = (b, Y // TH, X // TW)
        out[key] = out.get(key, 0) + k
    return out


def cell_of_pixel(b, y, x):
    """The one cell of a frame built here that can serve destination pixel (x, y): cells sit at even offsets from even tile origins."""
    return (int(b), int(x) - int(x) % 2, int(y) - int(y) % 2)


def redo_units(ws, n, h, w, cap):
    """The gather splat's redo list, decoded from the call's workspace (`_native._last_splat_ws`; ofl_kernels.hip, splat_pass_words):
    8 statistics words ([6]: units on the list), per-image flags and per-tile list lengths (each padded to 4 words), `cap` list slots
    per tile, then one (tile, b0 | b1 << 8 | fold << 16) pair per band unit.  -> [(b, ty, tx, b0, b1, fold)]."""
    ws = np.ascontiguousarray(ws).view(np.uint32)
    tx_n, ty_n = (w + TW - 1) // TW, (h + TH - 1) // TH
    tiles = n * tx_n * ty_n
    off = 8 + ((n + 3) & ~3) + ((tiles + 3) & ~3) + cap * tiles
    nu = int(ws[6])
    lst = ws[off:off + 2 * nu].reshape(nu, 2)
    out = []
    for t, v in lst:
        b, rem = divmod(int(t), tx_n * ty_n)
        ty, tx = divmod(rem, tx_n)
        out.append((b, ty, tx, int(v & 0xff), int((v >> 8) & 0xff), int((v >> 16) & 1)))
    return out
