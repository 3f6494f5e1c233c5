#!/usr/bin/env python3
"""Flow.photometric_stats and Flow.photometric on a batch of 1080p frames, next to the expression a user writes today
(Flow.invert('t').apply(other, return_valid_area=True) and eager torch operations) and to a device copy of as many bytes, all in one
process.

    python tools/bench_photometric.py [--batch 64] [--h 1080] [--w 1920] [--iters 50] [--warmup 5] [--blocks 5]
                                      [--out profiles/photometric_bench.json]

The flow is bench.py's smooth flow of sigma 8 read as an 's' flow, its mask has 20 % holes, the two frames are uniform noise, three
channels, float32 (first row) or uint8 (second row).  The algorithmic bytes of the forward pass are 8 (flow) + 1 (mask) + 4 C (img) +
4 C (other) per pixel (C each for uint8), computed from the shapes here: 33 B/px with float32 images, 4.4 GB at the default size,
several times the last-level cache.  Every figure is the median of `blocks` blocks of `iters` calls each, after `warmup` calls, by
HIP events; `*_spread_us` is the largest minus the smallest block.  Prints (and with --out writes) one JSON line: per image dtype
  stats_us, stats_gbs       Flow.photometric_stats(img, other): both kernels, the allocations and the torch arithmetic on the record
  fwd_bwd_us                Flow.photometric(img, other).sum().backward() with the vectors requiring a gradient
  torch_fwd_us              the same record from invert('t').apply(other, return_valid_area=True) and torch expressions
  torch_fwd_bwd_us          ... its mean, forward and backward (through the warp's autograd function)
  copy_us, copy_gbs         dst.copy_(src) of as many bytes in all (half read, half written) as the forward reads
  stats_vs_copy             stats_gbs / copy_gbs
  fwd_vs_torch, fwd_bwd_vs_torch       torch time / fused time
  fwd_beats_torch, fwd_bwd_beats_torch the fused median is below the torch median by more than the larger of the two spreads
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


def torch_record(flow, img, other, eps):
    """(count, sum, max) per image as a user computes them today: the warped image, then eager torch."""
    if img.dtype == torch.uint8:
        img, other = img.float() / 255.0, other.float() / 255.0
    warped, area = flow.invert('t').apply(other, return_valid_area=True)
    d = warped - img
    rho = torch.sqrt(d * d + eps * eps).mean(1)
    rho = rho * area
    return area.sum((1, 2)), rho.sum((1, 2)), rho.amax((1, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--h', type=int, default=1080)
    ap.add_argument('--w', type=int, default=1920)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    n, h, w, chan, eps = a.batch, a.h, a.w, 3, 1e-3
    gen = torch.Generator(device=dev).manual_seed(5)
    vecs = smooth_flow(n, h, w, 8.0, 1000, dev)
    mask = torch.rand((n, h, w), device=dev, generator=gen) > 0.2
    img32 = torch.rand((n, chan, h, w), device=dev, generator=gen)
    other32 = torch.rand((n, chan, h, w), device=dev, generator=gen)
    img8, other8 = (img32 * 255.0).to(torch.uint8), (other32 * 255.0).to(torch.uint8)
    flow = ofl.Flow(vecs, 's', mask)
    leaf = vecs.clone().requires_grad_()
    flow_g = ofl.Flow(leaf, 's', mask)
    px = n * h * w
    timed = lambda fn: events(fn, a.iters, a.warmup, a.blocks)
    res = {"op": "Flow.photometric_stats / Flow.photometric", "batch": n, "h": h, "w": w, "channels": chan, "ref": "s", "sigma": 8,
           "iters": a.iters, "warmup": a.warmup, "blocks": a.blocks, "eps": eps, "rows": []}
    for name, img, other in (("float32", img32, other32), ("uint8", img8, other8)):
        # algorithmic bytes read per pixel, forward
        bpp = vecs.element_size() * 2 + mask.element_size() + 2 * img.element_size() * chan
        src = torch.empty(bpp * px // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty(bpp * px // 2, dtype=torch.uint8, device=dev)
        copy_us, copy_spread = timed(lambda: dst.copy_(src))
        del src, dst
        row = {"images": name, "bytes_per_px_fwd": bpp, "bytes_read_per_call": bpp * px, "copy_us": copy_us,
               "copy_spread_us": copy_spread, "copy_gbs": round(2 * (bpp * px // 2) / copy_us / 1e3, 1)}
        s = flow.photometric_stats(img, other, eps=eps)
        row["kernel"] = _native.last_kernel_name()
        with torch.no_grad():
            count, total, _ = torch_record(flow, img, other, eps)
        row["count_new"], row["count_torch"] = int(s['count'].sum()), int(count.sum())
        row["mean_new"], row["mean_torch"] = float(s['photometric'].mean()), float((total.double() / count).mean())
        del count, total
        row["stats_us"], row["stats_spread_us"] = timed(lambda: flow.photometric_stats(img, other, eps=eps))
        row["stats_gbs"] = round(bpp * px / row["stats_us"] / 1e3, 1)

        def new_fwd_bwd():
            leaf.grad = None
            flow_g.photometric(img, other, eps=eps).sum().backward()

        row["fwd_bwd_us"], row["fwd_bwd_spread_us"] = timed(new_fwd_bwd)
        row["grad_kernel"] = _native.last_kernel_name()

        def torch_fwd_bwd():
            leaf.grad = None
            count, total, _ = torch_record(flow_g, img, other, eps)
            (total / count).sum().backward()

        with torch.no_grad():
            row["torch_fwd_us"], row["torch_fwd_spread_us"] = timed(lambda: torch_record(flow, img, other, eps))
        row["torch_fwd_bwd_us"], row["torch_fwd_bwd_spread_us"] = timed(torch_fwd_bwd)
        leaf.grad = None
        row["stats_vs_copy"] = round(row["stats_gbs"] / row["copy_gbs"], 3)
        row["fwd_vs_torch"] = round(row["torch_fwd_us"] / row["stats_us"], 2)
        row["fwd_bwd_vs_torch"] = round(row["torch_fwd_bwd_us"] / row["fwd_bwd_us"], 2)
        row["fwd_beats_torch"] = bool(row["torch_fwd_us"] - row["stats_us"] > max(row["stats_spread_us"], row["torch_fwd_spread_us"]))
        row["fwd_bwd_beats_torch"] = bool(row["torch_fwd_bwd_us"] - row["fwd_bwd_us"] >
                                          max(row["fwd_bwd_spread_us"], row["torch_fwd_bwd_spread_us"]))
        res["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + "\n")


if __name__ == '__main__':
    main()
