"""The loss sweep's comparison code for the SSIM kernels (a helper module, not a test): one launch of flow_ssim_kernel /
flow_ssim_grad_kernel on a frame of tests/frame_sweep.py against tests/ssim_oracle.py, with the bars of tests/test_gpu_ssim.py.
tests/loss_sweep.py and tests/frame_sweep.py are imported, not restated.

ofl_ssim.hip keeps the 64 x 16 tile and the 256-record chunk of ofl_census.hip's finish kernel (`geometry()` reads the three constants
out of the new source and `same_geometry_as_census()` holds them to the census ones), so the tile frames are
`frame_sweep.LOSS_TILE_FRAMES` and the chunk frames `frame_sweep.loop_frames()["census_finish"]`.  A variant is one of the frame's
`photometric_variants` -- what is no template argument (the ref, the channels, the mask) spread by the frame's key -- at a window."""
import numpy as np

import frame_sweep as fs
import loss_sweep as ls
import ssim_oracle as so
import test_gpu_ssim as tgs

WINDOWS = so.WINDOWS
ALL = ls.ALL


def geometry():
    """{kTileW, kTileH, kChunk} of ofl_ssim.hip"""
    text = fs._source("ofl_ssim.hip")
    return {k: fs._constant(text, k) for k in ("kTileW", "kTileH", "kChunk")}


def same_geometry_as_census():
    return geometry() == fs.loss_geometry()["census"]


def variants(h, w, window):
    """[dict(window, half, u8, ref, chan, masked)], one per (HALF, U8)"""
    return [dict(v, window=window) for v in fs.photometric_variants(h, w)]


def chunk_variant(h, w, window):
    """The variant a chunk frame runs at `window`: the frame's own (HALF, U8) number window % 4"""
    return variants(h, w, window)[window % 4]


def run(h, w, v, dev, images=ALL, backward=True, name_of=None):
    """dict(rec [n,8], map [n,h,w], loss [n], map_alone (a launch without records; with `name_of` only), grad [n,2,h,w] or None)"""
    from oflibpytorch_amd import _ssim
    ops = ls._dev_of(dev, *ls.photometric_operands(h, w, v, images))
    args = (so.sign_of(v["ref"]), v["window"], so.C1, so.C2)
    inst = "ILi%dE" % v["window"] + ls._b(v["half"]) + ls._b(v["u8"])
    out = dict(map_alone=None, grad=None)
    out["rec"], out["map"] = _ssim.flow_ssim(*ops, *args, want_map=True)
    ls._named(name_of, "flow_ssim_finish_kernel")
    out["loss"] = _ssim.ssim(*ops, *args)
    if name_of is not None:
        out["map_alone"] = _ssim.flow_ssim(*ops, *args, want_map=True, want_record=False)[1]
        ls._named(name_of, "flow_ssim_kernel" + inst)
    if backward:
        out["grad"] = _ssim.flow_ssim_grad(*ops, *args, ls._scale(ls._upstream(images), out["rec"][:, 0].cpu().numpy(), dev))
        ls._named(name_of, "flow_ssim_grad_kernel" + inst)
    return ls._numpy(out)


def check(h, w, v, dev, images=ALL, backward=True, name_of=None, tally=None):
    a, mask, img, other = ls.photometric_operands(h, w, v, images)
    want = so.compute(a, mask, img, other, v["ref"], v["window"])
    got = run(h, w, v, dev, images, backward, name_of)
    what = ls._what(h, w, v, images)
    rec, smap, known = got["rec"], got["map"], want["known"]
    assert rec.shape == (len(images), 8) and rec.dtype == np.float64, what
    ls.same_bits(smap, want["map"], what, "the map (n, y, x)")                              # +0 where not known
    if got["map_alone"] is not None:
        ls.same_bits(got["map_alone"], smap, what, "the map of a launch without records (n, y, x)")
    for k, name in ((0, "count"), (2, "max"), (3, "window pixels")):
        assert np.array_equal(rec[:, k], want["records"][:, k]), "%s: %s %s, expected %s" % (what, name, rec[:, k].tolist(),
                                                                                              want["records"][:, k].tolist())
    tgs.check_record_against_own_map(rec, smap, known, what)                                # sum within count * 2^-52, the rest +0
    ls.same_bits(got["loss"], ls._quotient(rec[:, 1], rec[:, 0]), what, "the loss against the quotient of its own record (n)")
    if backward:
        want_g, big_a = so.grad(a, mask, img, other, v["ref"], v["window"], so.C1, so.C2, tuple(ls._upstream(images)), res=want)
        ls.grad_within(got["grad"], want_g, so.grad_bound(want_g, big_a), ~known[:, None], what, tally)
    elif tally is not None:
        tally["launches"] = tally.get("launches", 0) + 1
    return got
