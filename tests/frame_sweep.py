"""The frame sweep's shared parts (not a conftest: test modules import it): the two lines of frames, their seeded content, and which
batch puts a swept frame into the size class of a recorded warp kernel.

FRAMES.  Width line: W in 2..9, 28..37, 60..69, 92..101, 124..133 at H = 17 and H = 66.  Height line: H in 2..5, 14..19, 30..34,
46..50, 62..67, 78..82, 126..131 at W = 36 (W % 4 == 0: the lean instantiations) and W = 35.  Always H, W >= 2.

CONTENT (`content(h, w)`, NumPy, seeded by the frame): FOUR distinct images, each with a flow, 9 source planes, 3 planes of a second
field (the addend, src_b), two masks with holes.  The flow is smooth (a few pixels, less on a short axis so that a 2-row frame keeps
a valid area) plus a shear, with a sign that changes along every border, so samples leave the frame across all four; named pixels
sample integer positions (fp32-exact through the normalisation) and the last row and column.  A launch of n images is those four
repeated cyclically (`batch`): the oracle runs on four images per frame, and an image-index or tile-decode error shows as a
neighbour's data.

REACH.  The launcher's thresholds count 32 x 16 tiles (g1) and 32 x 64 groups (g4) over the batch.  `choose()` restates warp_choose()
(ofl_kernels.hip) -- pinned on the CPU against every recorded case of tests/golden/warp_kernel_choice.json by
tests/test_frame_sweep_host.py, and on the GPU by the name of every swept launch.  `batch_for(case, h, w)` tries the batches on
either side of each threshold in that frame's g1 and g4 (rounded as `_sides()` of tests/test_gpu_warp_kernel_choice.py) and keeps the
smallest whose choice is the base case's; None where no batch can (H <= 16: g1 == g4, so g1 >= kColumnMinGroups > g4 never holds).

THE LOSS SWEEP (the last part of this file): the fused loss kernels and the backward of the scores on the same frames and content --
their geometry read from the sources, the operands, the frames that reach each state of each block loop, the kernels' index walks
restated, and the rule that spreads the variants over the frames."""
import json
import os
import re

import numpy as np

from special_values import sample_coord

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

WIDTHS = [w for lo, hi in ((2, 9), (28, 37), (60, 69), (92, 101), (124, 133)) for w in range(lo, hi + 1)]
HEIGHTS = [h for lo, hi in ((2, 5), (14, 19), (30, 34), (46, 50), (62, 67), (78, 82), (126, 131)) for h in range(lo, hi + 1)]
WIDTH_LINE = [(h, w) for h in (17, 66) for w in WIDTHS]
HEIGHT_LINE = [(h, w) for w in (36, 35) for h in HEIGHTS]
FRAMES = sorted(set(WIDTH_LINE + HEIGHT_LINE))
IMAGES = 4


# ------------------------------------------------------------------------------------------------------------------------------------
# content
# ------------------------------------------------------------------------------------------------------------------------------------
def exact_coords(size):
    """The integers of [0, size - 1] that sample_coord returns unchanged (special_values.exact_coords leaves the two ends out, and a frame
    of 2 or 3 then has none)."""
    k = np.arange(0, size, dtype=F32)
    return [int(v) for v in k[sample_coord(k, size) == k]]


_CONTENT = {}


def content(h, w):
    """dict(flow [4,2,h,w], src [4,9,h,w] (integers 0..255 as fp32: also the uint8 source; / 16 exact in fp16), other [4,3,h,w],
    m1, m2 [4,h,w] bool, named {name: [(y, x)]}) of the frame -- the same arrays on every call (read-only)."""
    if (h, w) in _CONTENT:
        return _CONTENT[(h, w)]
    rng = np.random.default_rng(1000003 * h + w)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    ax, ay = min(2.5, w / 16.0), min(2.5, h / 16.0)                       # amplitude: a few pixels, less on a short axis
    ty, tx = (ys / max(h - 1, 1)), (xs / max(w - 1, 1))
    flow = np.empty((IMAGES, 2, h, w), F32)
    for b in range(IMAGES):
        ph = 0.9 * b + rng.random(4) * 0.3
        # along a border the leading sine runs through 1.5 periods: both signs on every border; 0.4 of the amplitude for the other
        # axis' wave and 0.3 for the shear (u grows with y, v with x) leave its sign changes in place
        u = ax * (np.sin(2 * np.pi * (1.5 * ty + ph[0])) + 0.4 * np.cos(2 * np.pi * (tx + ph[1])) + 0.3 * (2 * ty - 1))
        v = ay * (np.sin(2 * np.pi * (1.5 * tx + ph[2])) + 0.4 * np.cos(2 * np.pi * (ty + ph[3])) - 0.3 * (2 * tx - 1))
        flow[b, 0], flow[b, 1] = u, v
    # named pixels (the same in every image, another target in each): integer sample positions, the last row, the last column
    ex, ey = exact_coords(w), exact_coords(h)
    spots = [(int(y), int(x)) for y, x in zip(*np.unravel_index(rng.permutation(h * w)[:min(12, h * w // 3)], (h, w)))]
    named = {"integer": [], "last_row": [], "last_col": [], "zero": []}
    for i, (y, x) in enumerate(spots):
        kind = ("integer", "last_row", "last_col", "zero")[i % 4]
        named[kind].append((y, x))
        for b in range(IMAGES):
            sx = ex[(3 * i + b) % len(ex)] if kind != "last_col" else w - 1
            sy = ey[(5 * i + b) % len(ey)] if kind != "last_row" else h - 1
            if kind == "zero":
                sx, sy = x, y
            elif kind == "last_row":
                sx = x - 0.25 if x >= 1 else x + 0.5
            elif kind == "last_col":
                sy = y - 0.25 if y >= 1 else y + 0.5
            flow[b, 0, y, x], flow[b, 1, y, x] = x - sx, y - sy
    src = rng.integers(0, 256, size=(IMAGES, 9, h, w)).astype(F32)
    other = (rng.integers(-256, 256, size=(IMAGES, 3, h, w)) / 32.0).astype(F32)
    masks = []
    for k in range(2):
        m = np.ones((IMAGES, h, w), bool)
        for b in range(IMAGES):
            while m[b].all() or any(np.array_equal(m[b], m[a]) for a in range(b)):      # (a tiny frame can draw the same holes twice)
                m[b] = True
                for _ in range(2):                                        # two rectangular holes, about 3 % of the frame each
                    hh, ww = max(1, h // 6), max(1, w // 6)
                    y0, x0 = int(rng.integers(0, h - hh + 1)), int(rng.integers(0, w - ww + 1))
                    m[b, y0:y0 + hh, x0:x0 + ww] = False
                m[b][rng.random((h, w)) < 0.02] = False
        masks.append(m)
    out = dict(flow=flow, src=src, other=other, m1=masks[0], m2=masks[1], named=named)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _CONTENT[(h, w)] = out
    return out


def sample_positions(flow):
    """(sx, sy) [n,h,w] in fp32 as the warp forms them."""
    n, _, h, w = flow.shape
    xs, ys = np.arange(w, dtype=F32)[None, None, :], np.arange(h, dtype=F32)[None, :, None]
    return sample_coord(xs - flow[:, 0], w), sample_coord(ys - flow[:, 1], h)


def batch(t4, n):
    """A launch's operand of n images from the four of a frame: repeated cyclically (torch tensor on any device, or NumPy)."""
    if isinstance(t4, np.ndarray):
        return t4[np.arange(n) % IMAGES]
    import torch
    return t4[torch.arange(n, device=t4.device) % IMAGES]


# ------------------------------------------------------------------------------------------------------------------------------------
# reach: the launcher's choice restated
# ------------------------------------------------------------------------------------------------------------------------------------
def constants():
    """The launcher's thresholds, read from the source that defines them (as tests/test_gpu_warp_kernel_choice.py does)."""
    with open(os.path.join(ROOT, 'oflibpytorch_amd', 'csrc', 'ofl_kernels.hip')) as fh:
        text = fh.read()
    col = int(re.search(r"constexpr unsigned kColumnMinGroups = (\d+)", text).group(1))

    def macro(name):
        body = re.search(r"^#define %s +(\(.*?\)|\S+)" % name, text, re.M).group(1)
        body = re.sub(r"(\d+)u\b", r"\1", body).replace("kColumnMinGroups", str(col))
        assert re.fullmatch(r"[\d\s()*+]+", body), body
        return int(eval(body))

    return dict(t1=macro("OFL_ROWS_T1_MAX"), t4=macro("OFL_ROWS_T4_MIN"), col=col, chan=macro("OFL_WARP_CHAN_WIDE_MIN"))


K = constants()
XCDS = 8
AUTO, GENERIC, PAIR, ONE_TILE, GROUPS, RECTANGLE, ROW_COLUMNS = 0, 1, 3, 4, 5, 6, 7


def tiles(n, h, w, tile_w, tile_h):
    t = -(-w // tile_w) * -(-h // tile_h) * n
    return -(-t // XCDS) * XCDS


def per_frame(h, w):
    """(g1 tiles, g4 groups) of one image."""
    return -(-w // 32) * -(-h // 16), -(-w // 32) * -(-h // 64)


def choose(kind, n, c, h, w, path, valid=False, addend=None, src_b=False, dst_flags=False, flags=False, to_u8=False, **_):
    """warp_choose() of ofl_kernels.hip for one launch: (family, tiles per block, lean, wide).  kind: plain / u8 / half / grad / x16."""
    if path == GENERIC or not (w >= 4 and h >= 2):
        return ("generic", 1, False, False)
    g1, g4 = tiles(n, h, w, 32, 16), tiles(n, h, w, 32, 64)
    lean = w % 4 == 0 and not to_u8 and not flags and h + 4 * w + 8 < 32760
    columns = path not in (PAIR, ONE_TILE)
    rows = columns and path != RECTANGLE
    automatic = path == AUTO
    rows_big = ("rows", 4, True, True)
    rows_small = ("rows", 1 if g1 < K["t1"] else 2, True, True)
    pair = ("pair", 2, False, False)
    if kind == "grad":
        if lean and rows:
            if g4 >= (K["t4"] if automatic else K["col"]) or path == ROW_COLUMNS:
                return rows_big
            if automatic:
                return rows_small
        return ("column", 4, False, False)
    add = addend is not None
    if c > 3:
        loop = ((kind == "plain" or (kind == "x16" and lean)) and c >= (7 if valid else 4) and w % 4 == 0 and not add and not src_b
                and not dst_flags and path != GROUPS)
        if not loop:          # launches of 3 channels, each with a choice of its own: the LAST one's (what last_kernel_name() reports),
            kw = dict(addend=addend, src_b=src_b, dst_flags=dst_flags, to_u8=to_u8)      # the mask and the flow's flag word ride with the first
            return choose(kind, n, (c - 1) % 3 + 1, h, w, path, valid=False, flags=False, **kw)
        if path != RECTANGLE and c >= 7 and lean:
            return ("chan_rows", 1, True, True)
        return ("chan", 1, lean, g1 >= K["chan"])
    if kind == "u8":
        if c in (1, 3) and w % 4 == 0 and rows and g4 >= K["col"]:
            return rows_big
        return pair
    if kind == "half" or src_b:
        if columns and g4 >= K["col"]:
            return rows_big if (lean and path != RECTANGLE) else ("column", 4, lean, False)
        return pair
    if dst_flags:
        if valid and rows and lean and g4 >= K["col"]:
            return rows_big
        return pair
    if add and c == 2 and not flags:
        is_flow = addend == "flow"
        if lean and rows and g4 >= (K["t4"] if (automatic and is_flow) else K["col"]):
            return rows_big
        if is_flow and lean and g4 < K["t4"] and automatic:
            return rows_small
        if g4 >= K["col"] and columns:
            return ("column", 4, lean, False)
    if path == ROW_COLUMNS and not add and lean:
        return rows_big
    if not add and automatic and lean:
        if g4 < K["t4"]:
            return rows_small
        if g4 < K["col"]:
            return rows_big
    if path == ONE_TILE or (path != PAIR and g1 < K["col"]):
        return ("column", 1, lean and valid, False)
    if not add and not flags and g4 >= K["col"] and path != PAIR:
        return rows_big if (lean and path != RECTANGLE) else ("column", 4, lean, True)
    return pair


def sides(threshold, per=1):
    at = -(-threshold // (8 * per)) * 8
    return at - 8, at


def batch_for(case, h, w):
    """The batch of the frame whose launch has the base case's choice: the base case's own threshold and side in this frame's g1, then
    in its g4 (n = threshold / tiles per image, rounded as `sides`), then the other thresholds' sides, smallest first; None where no
    batch has that choice."""
    want = choose(**case)
    opts = {k: v for k, v in case.items() if k not in ("n", "h", "w", "id")}
    g1f, g4f = per_frame(h, w)
    first, rest = [], {8}
    for thr in K.values():
        for base_per in set(per_frame(case["h"], case["w"])):
            for side in (0, 1):
                if sides(thr, base_per)[side] == case["n"]:
                    first += [sides(thr, g1f)[side], sides(thr, g4f)[side]]
        for per in (g1f, g4f):
            rest.update(sides(thr, per))
    for n in first + sorted(rest):
        if n >= IMAGES and choose(n=n, h=h, w=w, **opts) == want:
            return n
    return None


# ------------------------------------------------------------------------------------------------------------------------------------
# the recorded kernels
# ------------------------------------------------------------------------------------------------------------------------------------
def recorded_cases():
    """[(kernel name, base case)]: the smallest recorded case of each distinct (kind, kernel name) of tests/golden/warp_kernel_choice.json."""
    import test_gpu_warp_kernel_choice as kc
    by = {}
    for case in kc.CASES:
        by.setdefault((case["kind"], kc.RECORDED[case["id"]]), []).append(case)
    picked = [(key[1], min(cs, key=lambda c: (c["n"] * c["h"] * c["w"] * c["c"], c["id"]))) for key, cs in by.items()]
    return sorted(picked, key=lambda nc: nc[1]["id"])


def x16_cases():
    """Base cases for the table of tests/test_gpu_half_warp.py (EXPECTED: family, tiles per block, planes, VALID; fp16 and bf16): the
    launch of `_native._warp_bwd_x16` that reaches each, at that file's size classes."""
    out = []
    for valid in (False, True):
        for c in (1, 2, 3):
            for tiles_, n in ((1, sides(K["t1"])[0]), (2, sides(K["t1"])[1]), (4, sides(K["t4"])[1])):
                out.append((("rows", tiles_, c, valid), dict(kind="x16", h=16, w=32, n=n, c=c, path=AUTO, valid=valid)))
            out.append((("column", 1, c, valid), dict(kind="x16", h=16, w=30, n=sides(K["col"])[0], c=c, path=AUTO, valid=valid)))
            out.append((("pair", 2, c, valid), dict(kind="x16", h=64, w=30, n=sides(K["col"], 4)[1], c=c, path=AUTO, valid=valid)))
            out.append((("column", 4, c, valid), dict(kind="x16", h=16, w=30, n=sides(K["col"])[1], c=c, path=AUTO, valid=valid)))
        out.append((("chan_rows", 1, 0, valid), dict(kind="x16", h=8, w=16, n=8, c=9, path=AUTO, valid=valid)))
    out.append((("chan", 1, 0, False), dict(kind="x16", h=8, w=16, n=8, c=4, path=AUTO, valid=False)))
    return out


def tile_of(case):
    """(tile width, height of one block's column of tiles) whose residues a kernel must be run at: 32 x 16 tiles for the pair, one-tile
    and four-tile kernels on the rectangle, 64 x 16 where the choice says so, with row tables and in the 16-bit unit; times the tiles
    per block."""
    family, t, _, wide = choose(**case)
    tw = 64 if (wide or family in ("rows", "chan_rows") or case["kind"] == "x16") else 32
    return tw, 16 * max(t, 1)


def frames_for(case):
    """[(h, w, n)] of the swept frames (W >= 4: narrower ones are the generic kernel's) on which some batch gives the base case's
    choice.  The choice carries the lean flag, so a lean instantiation gets frames with W % 4 == 0 only; an instantiation that is not
    lean gets the other widths, and those with W % 4 == 0 too where the launcher sends them to it (a forced path, a uint8 source)."""
    out = []
    for h, w in FRAMES:
        n = batch_for(case, h, w) if w >= 4 else None
        if n is not None:
            out.append((h, w, n))
    return out


def _takes(case, widths):
    """Whether some batch of a 17-row frame of one of `widths` gives the base case's choice: 8 images, and both sides of every threshold
    in that frame's g1 and g4 (the batches `batch_for` tries)."""
    want = choose(**case)
    for w in widths:
        probes = {8} | {n for thr in K.values() for per in per_frame(17, w) for n in sides(thr, per) if n >= IMAGES}
        if any(choose(**dict(case, h=17, w=w, n=n)) == want for n in probes):
            return True
    return False


def residue_gaps(case, frames):
    """What the residue condition of the sweep still lacks for a kernel on `frames` (a list of strings, empty when it is met).  Heights:
    residues 0, 1 and T - 1 of the block's column height.  Widths: 0, 1 and T - 1 of the tile width and W % 4 in 1, 2, 3 -- for a kernel
    that the launcher gives widths with W % 4 == 0 only (a lean instantiation, the row tables, the channel loop) the nearest such: 0, 4
    and T - 4; for one that it gives the other widths only (its lean twin takes the rest) 1 and T - 1."""
    tw, th = tile_of(case)
    ws, hs = {w for _, w, _ in frames}, {h for h, _, _ in frames}
    ragged, aligned = _takes(case, (29, 30, 31)), _takes(case, (28, 32))
    assert ragged or aligned, "no width class takes %s: the probes of _takes() miss its size class" % (case.get("id", case),)
    gaps = ["H %% %d == %d" % (th, r) for r in (0, 1, th - 1) if not any(h % th == r for h in hs)]
    want = (0, 1, tw - 1) if (ragged and aligned) else (1, tw - 1) if ragged else (0, 4, tw - 4)
    gaps += ["W %% %d == %d" % (tw, r) for r in want if not any(w % tw == r for w in ws)]
    if ragged:
        gaps += ["W %% 4 == %d" % r for r in (1, 2, 3) if not any(w % 4 == r for w in ws)]
    return gaps


def load_table():
    with open(os.path.join(ROOT, 'tests', 'golden', 'warp_kernel_choice.json')) as fh:
        return json.load(fh)


# ------------------------------------------------------------------------------------------------------------------------------------
# the loss sweep: the fused loss kernels and the backward of the scores
# ------------------------------------------------------------------------------------------------------------------------------------
# ofl_smoothness.hip, ofl_photometric.hip, ofl_census.hip and flow_epe_grad_kernel of ofl_metrics.hip.  Every number below comes from
# `loss_geometry()`, which reads the constants out of the sources; tests/test_loss_sweep_host.py holds it to a literal table and proves,
# through a restatement of each kernel's index walk, that every frame of LOOP_FRAMES reaches the loop state it is listed for.
def _source(name):
    with open(os.path.join(ROOT, 'oflibpytorch_amd', 'csrc', name)) as fh:
        return fh.read()


def _constant(text, name):
    """`name = <number>` of a constexpr line (one line may define several: `constexpr int kTH = 8, kTW = 128;`)"""
    m = re.search(r"constexpr int [^;\n]*\b%s = (\d+)[,;]" % name, text)
    assert m, name
    return int(m.group(1))


_GEOMETRY = None


def loss_geometry():
    """{family: {constant: value}} read from the four sources; for the metrics also `grad_pixels`, the pixels one thread of
    flow_epe_grad_kernel takes per step (from the shift that forms its number of quads)."""
    global _GEOMETRY
    if _GEOMETRY is None:
        names = {"smoothness": ("kTH", "kTW", "kMaxBlocks", "kMaxGradBlocks"), "census": ("kTileW", "kTileH", "kChunk"),
                 "photometric": ("kThreads", "kMaxBlocks", "kMaxGradBlocks"), "metrics": ("kThreads", "kMaxBlocks", "kMaxGradBlocks")}
        out = {fam: {k: _constant(_source("ofl_%s.hip" % fam), k) for k in ks} for fam, ks in names.items()}
        body = re.search(r"flow_epe_grad_kernel\(ErrParams p\) \{(.*?)\n\}", _source("ofl_metrics.hip"), re.S).group(1)
        add, shift = map(int, re.search(r"quads = \(p\.hw \+ (\d+)\) >> (\d+)", body).groups())
        assert add == (1 << shift) - 1
        out["metrics"]["grad_pixels"] = 1 << shift
        _GEOMETRY = out
    return _GEOMETRY


LOSS_UPSTREAM = (0.75, -2.0, 1.0, 0.5)        # one upstream gradient per image of a frame (the oracles' own UPSTREAM has three)
_LOSS_INPUTS = {}


def loss_inputs(h, w):
    """The operands of the loss kernels from `content(h, w)`, the same arrays on every call (read-only): `flow` [4,2,h,w] fp32 and
    `flow16` as stored fp16, `mask` = m1, `img` = src[:, 0:3] / 255 (fp32; `img_u8` the same samples as uint8), `other` = src[:, 3:6] / 255
    (`other_u8`).  One channel: plane 0 alone (`images()`).  The smoothness guidance image is `img`.  A frame of one row or one column
    (smoothness alone takes those; `content()` needs H, W >= 2) is cut from the content of the frame with 2 in that axis."""
    if (h, w) not in _LOSS_INPUTS:
        t = content(max(h, 2), max(w, 2))
        cut = lambda a: np.ascontiguousarray(a[..., :h, :w])
        src = cut(t["src"])
        out = dict(flow=cut(t["flow"]), mask=cut(t["m1"]), img=src[:, 0:3] / F32(255), other=src[:, 3:6] / F32(255),
                   img_u8=src[:, 0:3].astype(np.uint8), other_u8=src[:, 3:6].astype(np.uint8))
        with np.errstate(over='ignore'):                                   # (a named pixel of a frame wider than 65 504 samples further
            out["flow16"] = out["flow"].astype(np.float16)                 # away than fp16 holds: inf, and the pixel is not known)
        assert out["img"].dtype == F32 and np.array_equal(out["img_u8"].astype(F32), src[:, 0:3])
        for a in out.values():
            a.setflags(write=False)
        _LOSS_INPUTS[(h, w)] = out
        if h * w > 1 << 16:                                                # a loop frame: its content is not kept twice
            _CONTENT.pop((max(h, 2), max(w, 2)), None)
    return _LOSS_INPUTS[(h, w)]


def images(t, u8, chan, images=None):
    """(img, other) of `loss_inputs` as uint8 or fp32, with 3 channels or plane 0 alone; `images`: those of the batch alone."""
    pair = (t["img_u8"], t["other_u8"]) if u8 else (t["img"], t["other"])
    sel = slice(None) if images is None else list(images)
    return tuple(np.ascontiguousarray(a[sel, :chan]) for a in pair)


# ---- the frames ----------------------------------------------------------------------------------------------------------------------
WIDE_LINE = [(17, w) for w in range(252, 262)]          # a 128-wide tile with a neighbour on both sides (and the 64-wide one: 4 or 5 across)
LOSS_TILE_FRAMES = sorted(set(FRAMES + WIDE_LINE))
SMOOTHNESS_ONLY = [(1, 5), (5, 1), (1, 1)]             # the other families refuse H or W < 2


def stream_sizes(*es):
    """The frames of the streaming sweep (tests/test_gpu_frame_sweep_stream.py) for one block step E or several: every h w from 4 to
    max E + 8 that a 2 x k or 3 x k frame has, and k E - 3 ... k E + 5 for k = 2, 3 and each E."""
    import test_gpu_frame_sweep_stream as st
    return st._sizes_of(list(es))


def photo_sizes():
    return stream_sizes(loss_geometry()["photometric"]["kThreads"])


def _isqrt(v):
    r = int(np.sqrt(v))
    while r * r > v:
        r -= 1
    while (r + 1) * (r + 1) <= v:
        r += 1
    return r


def loop_frames():
    """{kernel: [(state, h, w)]}: per kernel the smallest frames that reach each state of its block loop, from `loss_geometry()`.
    tests/test_loss_sweep_host.py asserts each state through the walks below."""
    g = loss_geometry()
    out = {}
    for name, cap in (("photometric_fwd", "kMaxBlocks"), ("photometric_bwd", "kMaxGradBlocks")):
        t = g["photometric"]["kThreads"]
        s = g["photometric"][cap] * t                                       # pixels of one round of the whole grid
        r = _isqrt(s) + 1
        frames = [("partial_second_round", r, r), ("step_x_zero", s // (2 * t) + 1, 2 * t), ("second_row", 2, s // 2 + 3),
                  ("step_y_zero", 2, s + 3)]
        if name == "photometric_fwd":
            frames += [("step_x_zero", s // t + 2, t), ("three_rounds", 3, 2 * s // 3 + 10)]
        out[name] = frames
    th, tw = g["smoothness"]["kTH"], g["smoothness"]["kTW"]
    for name, cap in (("smoothness_fwd", g["smoothness"]["kMaxBlocks"]), ("smoothness_bwd", g["smoothness"]["kMaxGradBlocks"])):
        rows = cap // 2 + 2                                                 # tile rows of a frame two tiles wide: four tiles over the cap,
                                                                            # a row of them inside the frame and the ragged last row
        out[name] = [("ragged_scalar", th * (rows - 1) + 1, tw + 1), ("ragged_vector", th * (rows - 1) + 1, tw + 4),
                     # three rounds, three tiles across (the middle one re-staged with a neighbour's pixels on both sides)
                     ("three_rounds", th * (-(-(2 * cap + 1) // 3) - 1) + 1, 2 * tw + 4)]
    cw, ch, chunk = g["census"]["kTileW"], g["census"]["kTileH"], g["census"]["kChunk"]
    # (a last tile row of ch / 2 + 1 rows, not of one: on a single last row the content's flow leaves the frame all along the stretch
    # of a few tiles, and the records of the last chunk would all be zero -- tests/test_loss_sweep_host.py asserts that they are not)
    out["census_finish"] = [("one_full_chunk", 2 * ch, cw * chunk // 2), ("full_chunk_and_two", ch + ch // 2 + 1, cw * chunk // 2 + 1),
                            ("two_full_chunks", 2 * ch, cw * chunk), ("three_chunks", 2 * ch + ch // 2 + 1, cw * (2 * chunk // 3) + 1)]
    e = g["metrics"]["kThreads"] * g["metrics"]["grad_pixels"]
    out["epe_grad"] = [("second_round", 2, g["metrics"]["kMaxGradBlocks"] * e // 2 + 3)]
    return out


def census_chunk_variant(h, w, patch):
    """The variant a chunk frame runs at `patch`: the frame's own (HALF, U8) number patch % 4, with q = 1 (the map bit for bit)"""
    return dict(photometric_variants(h, w)[patch % 4], patch=patch, q1=True)


# ---- the walks: each kernel's index arithmetic restated ------------------------------------------------------------------------------
def photometric_walk(h, w, backward):
    """flow_photometric_kernel's walk over an image, every lane of the grid at once: dict(rounds, step_x, step_y, wraps, straight,
    exact, first_round_wrap) -- the carried (x, y) is asserted equal to divmod(pix, w) at every pixel of every round; `wraps` /
    `straight` count the two branches of `if (x >= w)` over the carries whose round exists, `exact` those with x + step_x == w."""
    g = loss_geometry()["photometric"]
    t, cap = g["kThreads"], g["kMaxGradBlocks" if backward else "kMaxBlocks"]
    hw = h * w
    stride = min(-(-hw // t), cap) * t
    step_y, step_x = divmod(stride, w)
    pix = np.arange(stride, dtype=np.int64)
    y, x = np.divmod(pix, w)
    seen = np.zeros(hw, np.int32)
    out = dict(rounds=0, step_x=step_x, step_y=step_y, wraps=0, straight=0, exact=0, first_round_wrap=False)
    while True:
        live = pix < hw
        if not live.any():
            break
        assert np.array_equal(y[live] * w + x[live], pix[live]) and (x[live] < w).all() and (y[live] < h).all(), (h, w, out["rounds"])
        np.add.at(seen, pix[live], 1)
        nxt = pix + stride < hw
        x, y = x + step_x, y + step_y
        wrap = x >= w
        if nxt.any():
            out["wraps"] += int((wrap & nxt).sum())
            out["straight"] += int((~wrap & nxt).sum())
            out["exact"] += int(((x == w) & nxt).sum())
            out["first_round_wrap"] |= out["rounds"] == 0 and bool((wrap & nxt).any())
        x, y = np.where(wrap, x - w, x), np.where(wrap, y + 1, y)
        pix = pix + stride
        out["rounds"] += 1
    assert (seen == 1).all(), (h, w)
    return out


def smoothness_walk(h, w, backward):
    """flow_smoothness_kernel's walk: dict(tiles, tiles_x, tiles_y, nblk, rounds (of the busiest block), vec, later: the set of
    (ragged row, ragged column, neighbours on both sides in x, in y) of the tiles a block takes AFTER its first)."""
    g = loss_geometry()["smoothness"]
    th, tw, cap = g["kTH"], g["kTW"], g["kMaxGradBlocks" if backward else "kMaxBlocks"]
    tiles_x, tiles_y = -(-w // tw), -(-h // th)
    tiles = tiles_x * tiles_y
    nblk = min(tiles, cap)
    later, taken = set(), np.zeros(tiles, np.int32)
    for b in range(nblk):
        for k, tile in enumerate(range(b, tiles, nblk)):
            taken[tile] += 1
            ty, tx = divmod(tile, tiles_x)
            if k > 0:
                later.add((ty == tiles_y - 1 and h % th != 0, tx == tiles_x - 1 and w % tw != 0, 0 < tx < tiles_x - 1, 0 < ty < tiles_y - 1))
    assert (taken == 1).all()
    return dict(tiles=tiles, tiles_x=tiles_x, tiles_y=tiles_y, nblk=nblk, rounds=-(-tiles // nblk), vec=w % 4 == 0, later=later)


def census_walk(h, w):
    """flow_census_finish_kernel's chunks: dict(nblk, tiles_x, tiles_y, chunks [(base, cnt)])."""
    g = loss_geometry()["census"]
    tiles_x, tiles_y = -(-w // g["kTileW"]), -(-h // g["kTileH"])
    nblk = tiles_x * tiles_y
    chunks = [(base, min(nblk - base, g["kChunk"])) for base in range(0, nblk, g["kChunk"])]
    assert sum(c for _, c in chunks) == nblk
    return dict(nblk=nblk, tiles_x=tiles_x, tiles_y=tiles_y, chunks=chunks)


def census_block_counts(known):
    """The count field of flow_census_kernel's block records from the oracle's `known` [n,h,w]: [n, nblk], blocks in the kernel's order"""
    g = loss_geometry()["census"]
    n, h, w = known.shape
    ty, tx = -(-h // g["kTileH"]), -(-w // g["kTileW"])
    pad = np.zeros((n, ty * g["kTileH"], tx * g["kTileW"]), np.int64)
    pad[:, :h, :w] = known
    return pad.reshape(n, ty, g["kTileH"], tx, g["kTileW"]).sum((2, 4)).reshape(n, ty * tx)


def epe_grad_walk(h, w):
    """flow_epe_grad_kernel's walk over quads: dict(quads, stride, rounds, last: quads of the last round)."""
    g = loss_geometry()["metrics"]
    quads = -(-h * w // g["grad_pixels"])
    stride = min(-(-quads // g["kThreads"]), g["kMaxGradBlocks"]) * g["kThreads"]
    rounds = -(-quads // stride)
    return dict(quads=quads, stride=stride, rounds=rounds, last=quads - (rounds - 1) * stride)


# ---- the variants of a frame: a fixed rule keyed on the frame -------------------------------------------------------------------------
# Every frame runs every (HALF, U8) instantiation of the photometric kernel and every (ORDER, IMG) one of the smoothness kernel, so each
# meets every residue the frames have.  What is no template argument (the ref, the channels, the mask, fp16 storage for smoothness) is
# spread by the frame's key, another value for the next instantiation.  The census kernels are (PATCH, HALF, U8): a frame runs every
# (HALF, U8) at one patch each -- (h + w + j) % 3, so that neighbouring widths and heights give an instantiation its three residues --
# and at all three where the frame is no larger than the backward's halo of the widest patch in either axis.
CENSUS_PATCHES = (3, 5, 7)
TYPES = [(False, False), (False, True), (True, False), (True, True)]        # (fp16 vectors, uint8 images)


def frame_key(h, w):
    return 5 * h + w


def photometric_variants(h, w):
    """[dict(half, u8, ref, chan, masked)], one per (HALF, U8)."""
    k = frame_key(h, w)
    return [dict(half=hf, u8=u8, ref='st'[(k + j) % 2], chan=(3, 1)[(k // 2 + j) % 2], masked=(k // 4 + j) % 2 == 0)
            for j, (hf, u8) in enumerate(TYPES)]


def census_variants(h, w):
    """[dict(patch, half, u8, ref, chan, masked, q1)]: `q1`: q = 1 (the map bit for bit), else the default q."""
    out = []
    for j, v in enumerate(photometric_variants(h, w)):
        small = min(h, w) <= 2 * (max(CENSUS_PATCHES) // 2)
        for p in (CENSUS_PATCHES if small else (CENSUS_PATCHES[(h + w + j) % 3],)):
            out.append(dict(v, patch=p, q1=(frame_key(h, w) // 8 + j + p // 2) % 2 == 0))
    return out


SMOOTHNESS_KINDS = [(o, i) for o in (1, 2) for i in (None, "f32", "u8")]     # (ORDER, IMG)


def smoothness_variants(h, w):
    """[dict(order, kind, half, masked)], one per (ORDER, IMG)."""
    k = frame_key(h, w)
    return [dict(order=o, kind=i, half=(k + j) % 2 == 1, masked=(k // 2 + j) % 2 == 0) for j, (o, i) in enumerate(SMOOTHNESS_KINDS)]
