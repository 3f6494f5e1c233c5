#!/usr/bin/env python3
"""Flow.smoothness_stats and Flow.smoothness on a batch of 1080p frames, next to the torch expressions a user writes
today and to a device copy of as many bytes, all in one process.

    python tools/bench_smoothness.py [--batch 64] [--h 1080] [--w 1920] [--iters 50] [--warmup 5] [--out profiles/smoothness_bench.json]

The flow is a smooth field plus noise of sigma 0.3, its mask has 20 % holes, the guidance image is uniform noise with a step, three
channels, float32 (first row) or uint8 (second row).  The algorithmic bytes of the forward pass are 8 (flow) + 1 (mask) + 4 C (image;
C for uint8) per pixel, computed from the shapes here: 21 B/px with the float32 image, 2.8 GB at the default size, several times the
last-level cache.  A third row runs without an image (9 B/px, no exp): what the weights cost.  Times by HIP events.  Prints (and with --out writes) one JSON line: per image dtype and order
  stats_us, stats_gbs       Flow.smoothness_stats(img): both kernels, the allocations and the torch arithmetic on the record
  fwd_us                    Flow.smoothness(img) without a gradient
  fwd_bwd_us                Flow.smoothness(img).sum().backward() with the vectors requiring a gradient
  torch_fwd_us              the same per-image mean from torch expressions over the whole batch
  torch_fwd_bwd_us          ... forward and backward
  copy_us, copy_gbs         dst.copy_(src) of as many bytes in all (half read, half written) as the forward reads
  stats_vs_copy             stats_gbs / copy_gbs
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import oflibpytorch_amd as ofl  # noqa: E402
from oflibpytorch_amd import _native  # noqa: E402


def events(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3           # microseconds


def torch_smoothness(f, valid, img, order, alpha, eps):
    """The per-image mean of the valid terms, as a user writes it: shifted slices of the flow, the mask and the image."""
    if img is not None and img.dtype == torch.uint8:
        img = img.float() / 255.0
    total, count = 0.0, 0.0
    for axis in (3, 2):
        n = f.shape[axis]
        if order == 1:
            d = f.narrow(axis, 1, n - 1) - f.narrow(axis, 0, n - 1)
            ok = valid.narrow(axis - 1, 1, n - 1) & valid.narrow(axis - 1, 0, n - 1)
            g = None if img is None else (img.narrow(axis, 1, n - 1) - img.narrow(axis, 0, n - 1)).abs().mean(1)
        else:
            d = f.narrow(axis, 0, n - 2) - 2 * f.narrow(axis, 1, n - 2) + f.narrow(axis, 2, n - 2)
            ok = valid.narrow(axis - 1, 0, n - 2) & valid.narrow(axis - 1, 1, n - 2) & valid.narrow(axis - 1, 2, n - 2)
            g = None if img is None else (img.narrow(axis, 2, n - 2) - img.narrow(axis, 0, n - 2)).abs().mean(1) * 0.5
        t = torch.sqrt(d * d + eps * eps).sum(1)
        if g is not None:
            t = torch.exp(-alpha * g) * t
        total = total + (t * ok).sum((1, 2))
        count = count + ok.sum((1, 2))
    return total / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--h', type=int, default=1080)
    ap.add_argument('--w', type=int, default=1920)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    n, h, w, chan = a.batch, a.h, a.w, 3
    alpha, eps = 10.0, 1e-3
    gen = torch.Generator(device=dev).manual_seed(5)
    yy, xx = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing='ij')
    vecs = torch.empty((n, 2, h, w), device=dev)
    for i in range(n):
        vecs[i, 0], vecs[i, 1] = 2.0 * torch.sin(xx / 9.0 + i) + 0.05 * yy, 1.5 * torch.cos(yy / 7.0 - i) - 0.03 * xx
    vecs += torch.randn((n, 2, h, w), device=dev, generator=gen) * 0.3
    mask = torch.rand((n, h, w), device=dev, generator=gen) > 0.2
    img32 = torch.rand((n, chan, h, w), device=dev, generator=gen)
    img32[..., w // 2:] += 0.8
    img8 = (img32 * (255.0 / 1.8)).to(torch.uint8)
    flow = ofl.Flow(vecs, 't', mask)
    leaf = vecs.clone().requires_grad_()
    flow_g = ofl.Flow(leaf, 't', mask)
    px = n * h * w
    res = {"op": "Flow.smoothness_stats / Flow.smoothness", "batch": n, "h": h, "w": w, "channels": chan, "iters": a.iters,
           "warmup": a.warmup, "alpha": alpha, "eps": eps, "rows": []}
    for name, img in (("float32", img32), ("uint8", img8), ("none", None)):
        # algorithmic bytes read per pixel, forward
        bpp = vecs.element_size() * 2 + mask.element_size() + (0 if img is None else img.element_size() * chan)
        src = torch.empty(bpp * px // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty(bpp * px // 2, dtype=torch.uint8, device=dev)
        copy_us = round(events(lambda: dst.copy_(src), a.iters, a.warmup), 1)
        copy_gbs = round(2 * (bpp * px // 2) / copy_us / 1e3, 1)
        del src, dst
        for order in (1, 2):
            row = {"image": name, "order": order, "bytes_per_px_fwd": bpp, "bytes_read_per_call": bpp * px, "copy_us": copy_us,
                   "copy_gbs": copy_gbs}
            s = flow.smoothness_stats(img, order=order, alpha=alpha, eps=eps)
            row["kernel"] = _native.last_kernel_name()
            want = torch_smoothness(vecs, mask, img, order, alpha, eps)
            row["mean_new"] = float(s['smoothness'].mean())
            row["mean_torch"] = float(want.double().mean())
            del want
            row["stats_us"] = round(events(lambda: flow.smoothness_stats(img, order=order, alpha=alpha, eps=eps), a.iters, a.warmup), 1)
            row["stats_gbs"] = round(bpp * px / row["stats_us"] / 1e3, 1)
            row["fwd_us"] = round(events(lambda: flow.smoothness(img, order=order, alpha=alpha, eps=eps), a.iters, a.warmup), 1)

            def new_fwd_bwd():
                leaf.grad = None
                flow_g.smoothness(img, order=order, alpha=alpha, eps=eps).sum().backward()

            row["fwd_bwd_us"] = round(events(new_fwd_bwd, a.iters, a.warmup), 1)
            row["grad_kernel"] = _native.last_kernel_name()

            def torch_fwd_bwd():
                leaf.grad = None
                torch_smoothness(leaf, mask, img, order, alpha, eps).sum().backward()

            with torch.no_grad():
                row["torch_fwd_us"] = round(events(lambda: torch_smoothness(vecs, mask, img, order, alpha, eps), a.iters, a.warmup), 1)
            row["torch_fwd_bwd_us"] = round(events(torch_fwd_bwd, a.iters, a.warmup), 1)
            leaf.grad = None
            row["stats_vs_copy"] = round(row["stats_gbs"] / copy_gbs, 3)
            row["fwd_vs_torch"] = round(row["torch_fwd_us"] / row["fwd_us"], 1)
            row["fwd_bwd_vs_torch"] = round(row["torch_fwd_bwd_us"] / row["fwd_bwd_us"], 1)
            res["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + "\n")


if __name__ == '__main__':
    main()
