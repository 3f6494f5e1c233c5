#!/usr/bin/env python3
"""Flow.cost_volume on a batch of quarter-resolution 1080p feature maps, next to the composition it replaces
(Flow.invert('t').apply(other, return_valid_area=True), the mask, then D shifted-slice products with .sum(1) / C, stacked, in eager
torch) and to a device copy of as many bytes as the forward must move, all in one process.

    python tools/bench_cost_volume.py [--batch 8] [--channels 64] [--h 272] [--w 480] [--iters 10] [--torch-iters 3] [--warmup 2]
                                      [--blocks 5] [--radii 4 1] [--out profiles/cost_volume_bench.json]

The flow is bench.py's smooth flow of sigma 8 scaled by 1/4 and read as an 's' flow, its mask has 20 % holes, the two feature tensors
are uniform noise in [-1, 1), float32.  The algorithmic bytes of the forward pass are 8 (flow) + 1 (mask) + 4 C (feat) + 4 C (other)
read and 4 D (the volume) written per pixel, computed from the shapes here.  Every figure is the median of `blocks` blocks of `iters`
calls each (`torch-iters` for the composition), after `warmup` calls, by HIP events; `*_spread_us` is the largest minus the smallest
block.  Prints (and with --out writes) one JSON line: per radius
  fwd_us, fwd_gbs           Flow.cost_volume(feat, other): the kernel and the allocation of the volume
  fwd_bwd_us                ... and .backward(g) with feat, other and the vectors requiring a gradient
  torch_fwd_us              the same volume from invert('t').apply(other, return_valid_area=True) and torch expressions
  torch_fwd_bwd_us          ... forward and backward (through the warp's autograd function)
  copy_us, copy_gbs         dst.copy_(src) of as many bytes in all (half read, half written) as the forward reads and writes
  fwd_vs_copy               fwd_gbs / copy_gbs
  fwd_vs_torch, fwd_bwd_vs_torch       torch time / fused time
  fwd_beats_torch, fwd_bwd_beats_torch the fused median is below the torch median by more than the larger of the two spreads
  max_abs_diff              the largest difference between the two volumes (the composition's sum runs in another order)
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


def torch_volume(flow, feat, other, radius):
    """The volume as a user computes it today: the warped features, the valid area as a mask, D shifted-slice products."""
    warped, area = flow.invert('t').apply(other, return_valid_area=True)
    warped = warped * area[:, None]
    h, w = feat.shape[-2:]
    pad = torch.nn.functional.pad(warped, (radius, radius, radius, radius))
    c = feat.shape[1]
    return torch.stack([(feat * pad[..., radius + dy:radius + dy + h, radius + dx:radius + dx + w]).sum(1) / c
                        for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--channels', type=int, default=64)
    ap.add_argument('--h', type=int, default=272)
    ap.add_argument('--w', type=int, default=480)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--torch-iters', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--radii', type=int, nargs='+', default=[4, 1])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    n, h, w, chan = a.batch, a.h, a.w, a.channels
    gen = torch.Generator(device=dev).manual_seed(5)
    vecs = smooth_flow(n, h, w, 8.0, 1000, dev) * 0.25
    mask = torch.rand((n, h, w), device=dev, generator=gen) > 0.2
    feat = torch.rand((n, chan, h, w), device=dev, generator=gen) * 2 - 1
    other = torch.rand((n, chan, h, w), device=dev, generator=gen) * 2 - 1
    flow = ofl.Flow(vecs, 's', mask)
    leaf, feat_g, other_g = (t.clone().requires_grad_() for t in (vecs, feat, other))
    flow_g = ofl.Flow(leaf, 's', mask)
    px = n * h * w
    res = {"op": "Flow.cost_volume", "batch": n, "h": h, "w": w, "channels": chan, "features": "float32", "ref": "s", "sigma": 8,
           "flow_scale": 0.25, "iters": a.iters, "torch_iters": a.torch_iters, "warmup": a.warmup, "blocks": a.blocks, "rows": []}
    for radius in a.radii:
        d = (2 * radius + 1) ** 2
        # algorithmic bytes per pixel, forward: read and written
        bpp = vecs.element_size() * 2 + mask.element_size() + 2 * feat.element_size() * chan + 4 * d
        src = torch.empty(bpp * px // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty(bpp * px // 2, dtype=torch.uint8, device=dev)
        row = {"radius": radius, "offsets": d, "bytes_per_px_fwd": bpp, "bytes_per_call": bpp * px}
        row["copy_us"], row["copy_spread_us"] = events(lambda: dst.copy_(src), a.iters, a.warmup, a.blocks)
        row["copy_gbs"] = round(2 * (bpp * px // 2) / row["copy_us"] / 1e3, 1)
        del src, dst
        g = torch.rand((n, d, h, w), device=dev, generator=gen) * 2 - 1
        timed = lambda fn: events(fn, a.iters, a.warmup, a.blocks)
        slow = lambda fn: events(fn, a.torch_iters, min(a.warmup, 1), a.blocks)
        vol = flow.cost_volume(feat, other, radius=radius)
        row["kernel"] = _native.last_kernel_name()
        with torch.no_grad():
            row["max_abs_diff"] = float((vol - torch_volume(flow, feat, other, radius)).abs().max())
        del vol
        row["fwd_us"], row["fwd_spread_us"] = timed(lambda: flow.cost_volume(feat, other, radius=radius))
        row["fwd_gbs"] = round(bpp * px / row["fwd_us"] / 1e3, 1)
        row["fwd_vs_copy"] = round(row["fwd_gbs"] / row["copy_gbs"], 3)

        def clear():
            leaf.grad = feat_g.grad = other_g.grad = None

        def new_fwd_bwd():
            clear()
            flow_g.cost_volume(feat_g, other_g, radius=radius).backward(g)

        def torch_fwd_bwd():
            clear()
            torch_volume(flow_g, feat_g, other_g, radius).backward(g)

        row["fwd_bwd_us"], row["fwd_bwd_spread_us"] = timed(new_fwd_bwd)
        clear()
        torch.cuda.reset_peak_memory_stats(dev)
        with torch.no_grad():
            row["torch_fwd_us"], row["torch_fwd_spread_us"] = slow(lambda: torch_volume(flow, feat, other, radius))
        row["torch_fwd_bwd_us"], row["torch_fwd_bwd_spread_us"] = slow(torch_fwd_bwd)
        row["torch_peak_bytes"] = torch.cuda.max_memory_allocated(dev)
        clear()
        row["fwd_vs_torch"] = round(row["torch_fwd_us"] / row["fwd_us"], 2)
        row["fwd_bwd_vs_torch"] = round(row["torch_fwd_bwd_us"] / row["fwd_bwd_us"], 2)
        row["fwd_beats_torch"] = bool(row["torch_fwd_us"] - row["fwd_us"] > max(row["fwd_spread_us"], row["torch_fwd_spread_us"]))
        row["fwd_bwd_beats_torch"] = bool(row["torch_fwd_bwd_us"] - row["fwd_bwd_us"] >
                                          max(row["fwd_bwd_spread_us"], row["torch_fwd_bwd_spread_us"]))
        res["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del g
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + "\n")


if __name__ == '__main__':
    main()
