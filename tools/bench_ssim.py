#!/usr/bin/env python3
"""Flow.ssim_stats and Flow.ssim on a batch of 1080p frames, next to the expression a user writes today
(Flow.invert('t').apply(other, return_valid_area=True) and mask-weighted avg_pool2d expressions in eager torch) and to a device copy of
as many bytes, all in one process.

    python tools/bench_ssim.py [--batch 64] [--torch-batch 0] [--h 1080] [--w 1920] [--iters 50] [--torch-iters 50] [--warmup 5]
                               [--blocks 5] [--windows 3 7] [--out profiles/ssim_bench.json]

The flow is bench.py's smooth flow of sigma 8 read as an 's' flow, its mask has 20 % holes, the two frames are uniform noise, three
channels, float32.  The algorithmic bytes of the forward pass are 8 (flow) + 1 (mask) + 4 C (img) + 4 C (other) = 33 B/px, computed from
the shapes here.  The composition keeps, for its backward pass, some two dozen C x H x W float32 tensors: it runs at `--torch-batch`
images, by default the largest batch (up to --batch) whose estimate of 24 C + 16 H x W float32 tensors per image fits in 80 % of the
free device memory, and reports its peak (`torch_peak_bytes`); the fused call is measured at that batch and at --batch.  Every figure
is the median of `blocks` blocks of `iters` calls each (`torch-iters` for the composition), after `warmup` calls, by HIP events;
`*_spread_us` is the largest minus the smallest block.  Prints (and with --out writes) one JSON line: per window
  stats_us, stats_gbs       Flow.ssim_stats(img, other) at --batch: both kernels, the allocations and the torch arithmetic on the record
  fwd_bwd_us                Flow.ssim(img, other).sum().backward() at --batch with the vectors requiring a gradient
  small_stats_us, small_fwd_bwd_us     the same two at the composition's batch
  torch_fwd_us              the same record from invert('t').apply(other, return_valid_area=True) and torch expressions, at its batch
  torch_fwd_bwd_us          ... its mean, forward and backward (through the warp's autograd function)
  copy_us, copy_gbs         dst.copy_(src) of as many bytes in all (half read, half written) as the forward reads at --batch
  stats_vs_copy             stats_gbs / copy_gbs
  fwd_vs_torch, fwd_bwd_vs_torch       torch time / fused time, both at the composition's batch
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

C1, C2 = 1e-4, 9e-4


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


def torch_record(flow, img, other, window):
    """(count, sum, max, window pixels) per image as a user computes them today: the warped image, then box sums weighted by the valid
    area, each window normalised by the usable pixels it holds."""
    warped, area = flow.invert('t').apply(other, return_valid_area=True)
    us = area.float()[:, None]
    r = window // 2
    box = lambda t: torch.nn.functional.avg_pool2d(t, window, 1, r, divisor_override=1)
    cnt = box(us)
    den = cnt.clamp(min=1)
    mean = lambda t: box(us * t) / den
    mx, my = mean(warped), mean(img)
    sxx, syy, sxy = mean(warped * warped) - mx * mx, mean(img * img) - my * my, mean(warped * img) - mx * my
    ssim = (2 * mx * my + C1) * (2 * sxy + C2) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    rho = torch.clamp((1 - ssim) / 2, 0, 1).mean(1) * us[:, 0]
    return us.sum((1, 2, 3)), rho.sum((1, 2)), rho.amax((1, 2)), (cnt * us).sum((1, 2, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--torch-batch', type=int, default=0)
    ap.add_argument('--h', type=int, default=1080)
    ap.add_argument('--w', type=int, default=1920)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--torch-iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--windows', type=int, nargs='+', default=[3, 7])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    n, h, w, chan = a.batch, a.h, a.w, 3
    gen = torch.Generator(device=dev).manual_seed(5)
    vecs = smooth_flow(n, h, w, 8.0, 1000, dev)
    mask = torch.rand((n, h, w), device=dev, generator=gen) > 0.2
    img = torch.rand((n, chan, h, w), device=dev, generator=gen)
    other = torch.rand((n, chan, h, w), device=dev, generator=gen)
    flow = ofl.Flow(vecs, 's', mask)
    leaf = vecs.clone().requires_grad_()
    flow_g = ofl.Flow(leaf, 's', mask)
    px = n * h * w
    # algorithmic bytes read per pixel, forward
    bpp = vecs.element_size() * 2 + mask.element_size() + 2 * img.element_size() * chan
    src = torch.empty(bpp * px // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty(bpp * px // 2, dtype=torch.uint8, device=dev)
    copy_us, copy_spread = events(lambda: dst.copy_(src), a.iters, a.warmup, a.blocks)
    del src, dst
    res = {"op": "Flow.ssim_stats / Flow.ssim", "batch": n, "h": h, "w": w, "channels": chan, "images": "float32", "ref": "s",
           "sigma": 8, "iters": a.iters, "torch_iters": a.torch_iters, "warmup": a.warmup, "blocks": a.blocks, "c1": C1, "c2": C2,
           "bytes_per_px_fwd": bpp, "bytes_read_per_call": bpp * px, "copy_us": copy_us, "copy_spread_us": copy_spread,
           "copy_gbs": round(2 * (bpp * px // 2) / copy_us / 1e3, 1), "rows": []}
    for window in a.windows:
        kw = dict(window=window, c1=C1, c2=C2)
        timed = lambda fn: events(fn, a.iters, a.warmup, a.blocks)
        row = {"window": window}
        s = flow.ssim_stats(img, other, **kw)
        row["kernel"] = _native.last_kernel_name()
        row["stats_us"], row["stats_spread_us"] = timed(lambda: flow.ssim_stats(img, other, **kw))
        row["stats_gbs"] = round(bpp * px / row["stats_us"] / 1e3, 1)
        row["stats_vs_copy"] = round(row["stats_gbs"] / res["copy_gbs"], 3)

        def new_fwd_bwd(fl=flow_g, lf=leaf, im=img, ot=other):
            lf.grad = None
            fl.ssim(im, ot, **kw).sum().backward()

        row["fwd_bwd_us"], row["fwd_bwd_spread_us"] = timed(new_fwd_bwd)
        row["grad_kernel"] = _native.last_kernel_name()
        leaf.grad = None
        # the composition, at the largest batch its saved tensors leave room for
        free = torch.cuda.mem_get_info(dev)[0]
        fits = int(0.8 * free / ((24 * chan + 16) * h * w * 4))
        nt = a.torch_batch if a.torch_batch > 0 else max(1, min(n, fits))
        row["torch_batch"], row["free_bytes"] = nt, free
        torch.cuda.reset_peak_memory_stats(dev)
        small, small_leaf = ofl.Flow(vecs[:nt].clone(), 's', mask[:nt].clone()), vecs[:nt].clone().requires_grad_()
        small_g = ofl.Flow(small_leaf, 's', mask[:nt].clone())
        im, ot = img[:nt].contiguous(), other[:nt].contiguous()
        with torch.no_grad():
            count, total, _, terms = torch_record(small, im, ot, window)
        row["count_new"], row["count_torch"] = int(s['count'][:nt].sum()), int(count.sum())
        row["mean_new"], row["mean_torch"] = float(s['ssim'][:nt].mean()), float((total.double() / count).mean())
        row["fill_new"], row["fill_torch"] = float(s['fill'][:nt].mean()), float((terms.double() / (count * (window * window))).mean())
        del count, total, terms
        row["small_stats_us"], row["small_stats_spread_us"] = timed(lambda: small.ssim_stats(im, ot, **kw))
        row["small_fwd_bwd_us"], row["small_fwd_bwd_spread_us"] = timed(lambda: new_fwd_bwd(small_g, small_leaf, im, ot))
        small_leaf.grad = None

        def torch_fwd_bwd():
            small_leaf.grad = None
            count, total, _, _ = torch_record(small_g, im, ot, window)
            (total / count).sum().backward()

        slow = lambda fn: events(fn, a.torch_iters, min(a.warmup, 2), a.blocks)
        with torch.no_grad():
            row["torch_fwd_us"], row["torch_fwd_spread_us"] = slow(lambda: torch_record(small, im, ot, window))
        row["torch_fwd_bwd_us"], row["torch_fwd_bwd_spread_us"] = slow(torch_fwd_bwd)
        row["torch_peak_bytes"] = torch.cuda.max_memory_allocated(dev)
        small_leaf.grad = None
        row["fwd_vs_torch"] = round(row["torch_fwd_us"] / row["small_stats_us"], 2)
        row["fwd_bwd_vs_torch"] = round(row["torch_fwd_bwd_us"] / row["small_fwd_bwd_us"], 2)
        row["fwd_beats_torch"] = bool(row["torch_fwd_us"] - row["small_stats_us"] >
                                      max(row["small_stats_spread_us"], row["torch_fwd_spread_us"]))
        row["fwd_bwd_beats_torch"] = bool(row["torch_fwd_bwd_us"] - row["small_fwd_bwd_us"] >
                                          max(row["small_fwd_bwd_spread_us"], row["torch_fwd_bwd_spread_us"]))
        res["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del small, small_g, small_leaf, im, ot
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + "\n")


if __name__ == '__main__':
    main()
