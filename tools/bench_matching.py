#!/usr/bin/env python3
"""Flow.from_matching next to the eager composition in fp32 torch (matmul into the (H W)^2 volume, softmax over it, matmul
with the coordinate grid), all in one process.

    python tools/bench_matching.py [--case full|crop|both] [--batch 8] [--channels 128] [--iters 3] [--warmup 1] [--blocks 5]
                                   [--out profiles/matching_bench.json]

Cases: `full` 135 x 240 (eighth-resolution 1080p) and `crop` 48 x 96 (GMFlow's training crop at 1/8), B = 8 and C = 128 by default; the
features are N(0, 1), float32, the upstream gradient uniform in [-1, 1).  Every figure is the median of `blocks` blocks of `iters` calls
each, after `warmup` calls, by HIP events; `*_spread_us` is the largest minus the smallest block.  Peak memory is
torch.cuda.max_memory_allocated beyond what was allocated before the call (the inputs).  The eager composition runs on the first
`eager_images` images: the whole batch, or at 135 x 240 as many as leave its volume, softmax and gradient (three volumes of 4 (H W)^2
bytes an image) under half the device's free memory; its times and peaks are also given per image, and the ratios compare per image.
Prints one JSON line per case and with --out writes {case: result} (an existing file keeps its other cases):
  fwd_us, fwd_peak_bytes                     Flow.from_matching(feat, other, 's', return_prob=True): one launch, the allocations, the Flow
  fwd_bwd_us, fwd_bwd_peak_bytes             ... and .vecs.backward(g) with both feature tensors requiring a gradient
  fwd_tflops, fwd_frac_nofma_peak            2 C (H W)^2 flops an image over fwd_us; over 78.65 TFLOPS, the no-FMA half of the vector peak
  eager_fwd_us, eager_fwd_peak_bytes, ...    the eager composition on `eager_images` images, and its forward plus backward
  time_ratio_fwd, time_ratio_fwd_bwd         fused over eager, per image;  mem_ratio_fwd, mem_ratio_fwd_bwd likewise (peak bytes)
  max_abs_diff, max_abs_diff_prob, max_abs_diff_d_feat, max_abs_diff_d_other     the largest differences between the two results
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

CASES = {"full": (135, 240), "crop": (48, 96)}
NOFMA_PEAK_TFLOPS = 157.3 / 2


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


def eager_expression(feat, other):
    """GMFlow's global_correlation_softmax: (flow [n,2,h,w] of an 's' flow, prob [n,h,w])"""
    n, c, h, w = feat.shape
    corr = torch.matmul(feat.view(n, c, h * w).transpose(1, 2), other.view(n, c, h * w)) / (c ** 0.5)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=feat.dtype, device=feat.device), torch.arange(w, dtype=feat.dtype, device=feat.device),
                            indexing='ij')
    grid = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1)
    p = torch.softmax(corr, dim=2)
    flow = (torch.matmul(p, grid) - grid[None]).transpose(1, 2).reshape(n, 2, h, w)
    return flow, p.max(dim=2).values.view(n, h, w)


def peak(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated(dev) - base


def measure(name, n, c, a, dev):
    h, w = CASES[name]
    gen = torch.Generator(device=dev).manual_seed(11)
    feat = torch.randn((n, c, h, w), device=dev, generator=gen)
    other = torch.randn((n, c, h, w), device=dev, generator=gen)
    g = torch.rand((n, 2, h, w), device=dev, generator=gen) * 2 - 1
    timed = lambda fn: events(fn, a.iters, a.warmup, a.blocks)
    volume = 4 * (h * w) ** 2
    res = {"case": name, "batch": n, "channels": c, "h": h, "w": w, "volume_bytes_per_image": volume}
    fused = lambda: ofl.Flow.from_matching(feat, other, 's', return_prob=True)
    (flow, prob), res["fwd_peak_bytes"] = peak(fused, dev)
    res["kernel"] = _native.last_kernel_name()
    res["fwd_us"], res["fwd_spread_us"] = timed(fused)
    res["fwd_tflops"] = round(2.0 * c * (h * w) ** 2 * n / res["fwd_us"] / 1e6, 2)
    res["fwd_frac_nofma_peak"] = round(res["fwd_tflops"] / NOFMA_PEAK_TFLOPS, 4)
    f_g, o_g = feat.clone().requires_grad_(), other.clone().requires_grad_()

    def fused_fwd_bwd():
        f_g.grad, o_g.grad = None, None
        ofl.Flow.from_matching(f_g, o_g, 's').vecs.backward(g)

    _, res["fwd_bwd_peak_bytes"] = peak(fused_fwd_bwd, dev)
    res["fwd_bwd_us"], res["fwd_bwd_spread_us"] = timed(fused_fwd_bwd)
    d_fused = (f_g.grad.clone(), o_g.grad.clone())
    f_g.grad, o_g.grad = None, None
    # the eager composition, on as many images as fit
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info(dev)[0]
    k = max(1, min(n, int(free // 2 // (3 * volume))))
    res["device_free_bytes"], res["eager_images"] = int(free), k
    fe, oe, ge = f_g[:k].detach().clone().requires_grad_(), o_g[:k].detach().clone().requires_grad_(), g[:k].contiguous()
    with torch.no_grad():
        (ref, ref_prob), res["eager_fwd_peak_bytes"] = peak(lambda: eager_expression(fe, oe), dev)
        res["max_abs_diff"] = float((flow.vecs[:k] - ref).abs().max())
        res["max_abs_diff_prob"] = float((prob[:k] - ref_prob).abs().max())
        del ref, ref_prob
        res["eager_fwd_us"], res["eager_fwd_spread_us"] = timed(lambda: eager_expression(fe, oe))

    def eager_fwd_bwd():
        fe.grad, oe.grad = None, None
        eager_expression(fe, oe)[0].backward(ge)

    _, res["eager_fwd_bwd_peak_bytes"] = peak(eager_fwd_bwd, dev)
    res["eager_fwd_bwd_us"], res["eager_fwd_bwd_spread_us"] = timed(eager_fwd_bwd)
    res["max_abs_diff_d_feat"] = float((d_fused[0][:k] - fe.grad).abs().max())
    res["max_abs_diff_d_other"] = float((d_fused[1][:k] - oe.grad).abs().max())
    for key in ("fwd", "fwd_bwd"):
        res["time_ratio_" + key] = round((res[key + "_us"] / n) / (res["eager_" + key + "_us"] / k), 3)
        res["mem_ratio_" + key] = round((res[key + "_peak_bytes"] / n) / (res["eager_" + key + "_peak_bytes"] / k), 6)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='both', choices=('full', 'crop', 'both'))
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--channels', type=int, default=128)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    done = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            done = json.load(f)
    for name in (('crop', 'full') if a.case == 'both' else (a.case,)):
        res = {"op": "Flow.from_matching", "features": "float32", "ref": "s", "iters": a.iters, "warmup": a.warmup, "blocks": a.blocks}
        res.update(measure(name, a.batch, a.channels, a, dev))
        print(json.dumps(res), flush=True)
        done[name] = res
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(done, indent=1, sort_keys=True) + "\n")


if __name__ == '__main__':
    main()
