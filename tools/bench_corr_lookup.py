#!/usr/bin/env python3
"""Flow.corr_lookup on a batch of eighth-resolution 1080p feature maps, next to the all-pairs composition it stands in
for (RAFT's CorrBlock in eager torch: matmul of the two feature maps over sqrt(C), avg_pool2d pyramid, grid_sample per level) and to a
device copy of as many bytes as the forward must move, all in one process.

    python tools/bench_corr_lookup.py [--batch 8] [--channels 256] [--h 135] [--w 240] [--radius 4] [--levels 4] [--iters 3]
                                      [--warmup 1] [--blocks 5] [--pairs-batch 2] [--out profiles/corr_lookup_bench.json]

The flow is bench.py's smooth flow of sigma 8 scaled by 1/8 and read as an 's' flow, its mask has 20 % holes, the two feature tensors
are uniform noise in [-1, 1), float32.  The pyramid of `other` is pooled once, outside the timed region, as a training loop does for its
12 to 32 lookups.  The algorithmic bytes of the forward are 8 (flow) + 1 (mask) + 4 C (feat) + 4 C (1 + 1/4 + ...) (the levels) read
and 4 L D written per pixel.  Every figure is the median of `blocks` blocks of `iters` calls each, after `warmup` calls, by HIP events;
`*_spread_us` is the largest minus the smallest block.  The all-pairs volume of the whole batch is (H W)^2 floats per image and a
third more with its pyramid, and as much again for its gradient: the composition runs on the first `pairs-batch` images only (its
figures are per call on that batch; `*_per_image_us` divides by it).  Prints (and with --out writes) one JSON line:
  fwd_us, fwd_gbs, fwd_peak_bytes          Flow.corr_lookup(feat, levels): L launches and the allocation of the result
  fwd_bwd_us, fwd_bwd_peak_bytes           ... and .backward(g) with feat and every level requiring a gradient
  pyramid_us                               corr_pyramid(other, L), once per pair of frames
  copy_us, copy_gbs, fwd_vs_copy           dst.copy_(src) of as many bytes in all as the forward reads and writes
  pairs_build_us, pairs_build_peak_bytes   the all-pairs volume and its pyramid, once per pair of frames
  pairs_fwd_us                             one lookup on that pyramid (grid_sample per level, concatenated)
  pairs_fwd_bwd_us, pairs_peak_bytes       ... and its backward into the pyramid's levels (not through the build)
  max_abs_diff                             the largest difference between the two lookups on the images both computed
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import oflibpytorch_amd as ofl  # noqa: E402
from bench import smooth_flow  # noqa: E402
from oflibpytorch_amd import _native  # noqa: E402


def events(fn, iters, warmup, blocks):
    """(median, spread) in microseconds per call over `blocks` blocks of `iters` calls"""
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / iters * 1e3)
    times.sort()
    return round(times[len(times) // 2], 1), round(times[-1] - times[0], 1)


def pairs_build(feat, other, levels):
    """RAFT's CorrBlock.__init__: the all-pairs volume [N H W, 1, H, W] and its pooled pyramid"""
    n, c, h, w = feat.shape
    corr = torch.matmul(feat.reshape(n, c, h * w).transpose(1, 2), other.reshape(n, c, h * w)) / float(c) ** 0.5
    pyr = [corr.reshape(n * h * w, 1, h, w)]
    for _ in range(levels - 1):
        pyr.append(torch.nn.functional.avg_pool2d(pyr[-1], 2, 2))
    return pyr


def pairs_lookup(pyr, coords, radius, n, h, w):
    """RAFT's CorrBlock.__call__: coords [N, 2, H, W] (x, y) in pixels of level 0"""
    d = torch.linspace(-radius, radius, 2 * radius + 1, device=coords.device)
    delta = torch.stack(torch.meshgrid(d, d, indexing='ij'), -1)[None]                        # [1, 2r+1, 2r+1, 2]: the x offset first
    centre = coords.permute(0, 2, 3, 1).reshape(n * h * w, 1, 1, 2)
    out = []
    for l, corr in enumerate(pyr):
        hl, wl = corr.shape[-2:]
        at = centre / 2 ** l + delta
        grid = torch.stack([2 * at[..., 0] / (wl - 1) - 1, 2 * at[..., 1] / (hl - 1) - 1], -1)
        out.append(torch.nn.functional.grid_sample(corr, grid, align_corners=True).reshape(n, h, w, -1))
    return torch.cat(out, -1).permute(0, 3, 1, 2).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--channels', type=int, default=256)
    ap.add_argument('--h', type=int, default=135)
    ap.add_argument('--w', type=int, default=240)
    ap.add_argument('--radius', type=int, default=4)
    ap.add_argument('--levels', type=int, default=4)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--pairs-batch', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    n, h, w, chan, radius, levels = a.batch, a.h, a.w, a.channels, a.radius, a.levels
    nb = min(a.pairs_batch, n)
    gen = torch.Generator(device=dev).manual_seed(5)
    vecs = smooth_flow(n, h, w, 8.0, 1000, dev) * 0.125
    mask = torch.rand((n, h, w), device=dev, generator=gen) > 0.2
    feat = torch.rand((n, chan, h, w), device=dev, generator=gen) * 2 - 1
    other = torch.rand((n, chan, h, w), device=dev, generator=gen) * 2 - 1
    d = (2 * radius + 1) ** 2
    g = torch.rand((n, levels * d, h, w), device=dev, generator=gen) * 2 - 1
    flow = ofl.Flow(vecs, 's', mask)
    px = n * h * w
    timed = lambda fn: events(fn, a.iters, a.warmup, a.blocks)
    res = {"op": "Flow.corr_lookup", "batch": n, "h": h, "w": w, "channels": chan, "radius": radius, "levels": levels, "features": "float32",
           "ref": "s", "sigma": 8, "flow_scale": 0.125, "iters": a.iters, "warmup": a.warmup, "blocks": a.blocks, "pairs_batch": nb}

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated(dev) - base

    # ---- the fused lookup ------------------------------------------------------------------------------------------------------------
    res["pyramid_us"], res["pyramid_spread_us"] = timed(lambda: ofl.corr_pyramid(other, levels))
    pyr = ofl.corr_pyramid(other, levels)
    level_px = sum(int(t.shape[-2]) * int(t.shape[-1]) for t in pyr) * n
    nbytes = (8 + 1 + 4 * chan + 4 * levels * d) * px + 4 * chan * level_px
    res["bytes_per_call"] = nbytes
    out, res["fwd_peak_bytes"] = peak(lambda: flow.corr_lookup(feat, pyr, radius=radius))
    res["kernel"] = _native.last_kernel_name()
    res["fwd_us"], res["fwd_spread_us"] = timed(lambda: flow.corr_lookup(feat, pyr, radius=radius))
    res["fwd_gbs"] = round(nbytes / res["fwd_us"] / 1e3, 1)
    feat_g = feat.clone().requires_grad_()
    pyr_g = [t.clone().requires_grad_() for t in pyr]

    def fused_fwd_bwd():
        feat_g.grad = None
        for t in pyr_g:
            t.grad = None
        flow.corr_lookup(feat_g, pyr_g, radius=radius).backward(g)

    _, res["fwd_bwd_peak_bytes"] = peak(fused_fwd_bwd)
    res["fwd_bwd_us"], res["fwd_bwd_spread_us"] = timed(fused_fwd_bwd)
    feat_g.grad = None
    for t in pyr_g:
        t.grad = None
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    res["copy_us"], res["copy_spread_us"] = timed(lambda: dst.copy_(src))
    res["copy_gbs"] = round(2 * (nbytes // 2) / res["copy_us"] / 1e3, 1)
    res["fwd_vs_copy"] = round(res["fwd_gbs"] / res["copy_gbs"], 4)
    del src, dst
    print(json.dumps(res), file=sys.stderr, flush=True)

    # ---- the all-pairs composition on the first images -------------------------------------------------------------------------------
    res["pairs_volume_bytes_per_image"] = 4 * (h * w) ** 2
    ys, xs = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing='ij')
    coords = torch.stack([xs, ys])[None] + vecs[:nb]                                           # an 's' flow: p + a(p)
    with torch.no_grad():
        big, res["pairs_build_peak_bytes"] = peak(lambda: pairs_build(feat[:nb], other[:nb], levels))
        del big
        res["pairs_build_us"], res["pairs_build_spread_us"] = timed(lambda: pairs_build(feat[:nb], other[:nb], levels))
        big = pairs_build(feat[:nb], other[:nb], levels)
        ref = pairs_lookup(big, coords, radius, nb, h, w) * mask[:nb, None]
        res["max_abs_diff"] = float((out[:nb] - ref).abs().max())
        del ref, out
        res["pairs_fwd_us"], res["pairs_fwd_spread_us"] = timed(lambda: pairs_lookup(big, coords, radius, nb, h, w))
    for t in big:
        t.requires_grad_()

    def pairs_fwd_bwd():
        for t in big:
            t.grad = None
        pairs_lookup(big, coords, radius, nb, h, w).backward(g[:nb])

    _, res["pairs_fwd_bwd_peak_bytes"] = peak(pairs_fwd_bwd)
    res["pairs_fwd_bwd_us"], res["pairs_fwd_bwd_spread_us"] = timed(pairs_fwd_bwd)
    res["pairs_peak_bytes"] = res["pairs_fwd_bwd_peak_bytes"] + sum(t.numel() * 4 for t in big)
    for key in ("pairs_build_us", "pairs_fwd_us", "pairs_fwd_bwd_us"):
        res[key.replace("_us", "_per_image_us")] = round(res[key] / nb, 1)
    for key in ("fwd_us", "fwd_bwd_us"):
        res[key.replace("_us", "_per_image_us")] = round(res[key] / n, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + "\n")


if __name__ == '__main__':
    main()
