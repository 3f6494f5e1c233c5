#!/usr/bin/env python3
"""Flow.propagate next to the eager compositions in fp32 torch, all in one process: the global form against matmul into
the (H W)^2 volume, softmax over it and matmul with the vectors; the local form against GMFlow's unfold of the key and of the flow.

    python tools/bench_propagate.py [--case NAME|all] [--batch 8] [--channels 128] [--iters 3] [--warmup 1] [--blocks 5]
                                    [--out profiles/propagate_bench.json]

Cases: `global_full` 135 x 240 (eighth-resolution 1080p) and `global_crop` 48 x 96 (GMFlow's training crop at 1/8); `local_r1` and
`local_r4` at 270 x 480 (quarter resolution) with radius 1 and 4; B = 8 and C = 128 by default.  The features are N(0, 1), float32, the
vectors N(0, 4), the upstream gradient uniform in [-1, 1), the flow's mask all True and considered (the kernels read it).  Every figure
is the median of `blocks` blocks of `iters` calls each, after `warmup` calls, by HIP events; `*_spread_us` is the largest minus the
smallest block.  Peak memory is torch.cuda.max_memory_allocated beyond what was allocated before the call (the inputs).  The eager
composition runs on the first `eager_images` images: the whole batch, or as many as leave its intermediates (three volumes of 4 (H W)^2
bytes an image; three unfolded keys of 4 (2 r + 1)^2 C H W bytes) under half the device's free memory; the ratios compare per image.
Prints one JSON line per case and with --out writes {case: result} (an existing file keeps its other cases):
  fwd_us, fwd_peak_bytes                     flow.propagate(query, key, radius): one launch, the allocations, the Flow
  fwd_bwd_us, fwd_bwd_peak_bytes             ... and .vecs.backward(g) with query, key and the vectors requiring a gradient
  fwd_tflops                                 2 C T flops a pixel over fwd_us, T = H W (global) or (2 r + 1)^2 (local)
  eager_fwd_us, eager_fwd_peak_bytes, ...    the eager composition on `eager_images` images, and its forward plus backward
  time_ratio_fwd, time_ratio_fwd_bwd         fused over eager, per image;  mem_ratio_fwd, mem_ratio_fwd_bwd likewise (peak bytes)
  max_abs_diff, max_abs_diff_d_query, max_abs_diff_d_key, max_abs_diff_d_flow     the largest differences between the two results
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import oflibpytorch_amd as ofl  # noqa: E402

CASES = {"global_crop": (48, 96, None), "global_full": (135, 240, None), "local_r1": (270, 480, 1), "local_r4": (270, 480, 4)}


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


def eager_expression(vecs, query, key, radius):
    """GMFlow's SelfAttnPropagation without its projections: the global form, or the local form by unfold with zero padding"""
    n, c, h, w = query.shape
    if radius is None:
        corr = torch.matmul(query.view(n, c, h * w).transpose(1, 2), key.view(n, c, h * w)) / (c ** 0.5)
        return torch.matmul(torch.softmax(corr, dim=2), vecs.view(n, 2, h * w).transpose(1, 2)).transpose(1, 2).reshape(n, 2, h, w)
    k = 2 * radius + 1
    kw = torch.nn.functional.unfold(key, k, padding=radius).view(n, c, k * k, h * w)
    corr = (query.view(n, c, 1, h * w) * kw).sum(1) / (c ** 0.5)
    fw = torch.nn.functional.unfold(vecs, k, padding=radius).view(n, 2, k * k, h * w)
    return (torch.softmax(corr, dim=1)[:, None] * fw).sum(2).view(n, 2, h, w)


def peak(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated(dev) - base


def measure(name, n, c, a, dev):
    h, w, radius = CASES[name]
    gen = torch.Generator(device=dev).manual_seed(11)
    query = torch.randn((n, c, h, w), device=dev, generator=gen)
    key = torch.randn((n, c, h, w), device=dev, generator=gen)
    vecs = torch.randn((n, 2, h, w), device=dev, generator=gen) * 2
    g = torch.rand((n, 2, h, w), device=dev, generator=gen) * 2 - 1
    timed = lambda fn: events(fn, a.iters, a.warmup, a.blocks)
    steps = h * w if radius is None else (2 * radius + 1) ** 2
    inter = 4 * (h * w) ** 2 if radius is None else 4 * steps * c * h * w
    res = {"case": name, "batch": n, "channels": c, "h": h, "w": w, "radius": radius, "eager_intermediate_bytes_per_image": inter}
    flow = ofl.Flow(vecs, 't')
    fused = lambda: flow.propagate(query, key, radius)
    out, res["fwd_peak_bytes"] = peak(fused, dev)
    res["fwd_us"], res["fwd_spread_us"] = timed(fused)
    res["fwd_tflops"] = round(2.0 * c * steps * h * w * n / res["fwd_us"] / 1e6, 2)
    q_g, k_g, v_g = query.clone().requires_grad_(), key.clone().requires_grad_(), vecs.clone().requires_grad_()

    def fused_fwd_bwd():
        q_g.grad, k_g.grad, v_g.grad = None, None, None
        ofl.Flow(v_g, 't').propagate(q_g, k_g, radius).vecs.backward(g)

    _, res["fwd_bwd_peak_bytes"] = peak(fused_fwd_bwd, dev)
    res["fwd_bwd_us"], res["fwd_bwd_spread_us"] = timed(fused_fwd_bwd)
    d_fused = (q_g.grad.clone(), k_g.grad.clone(), v_g.grad.clone())
    q_g.grad, k_g.grad, v_g.grad = None, None, None
    # the eager composition, on as many images as fit
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info(dev)[0]
    k = max(1, min(n, int(free // 2 // (3 * inter))))
    res["device_free_bytes"], res["eager_images"] = int(free), k
    qe, ke, ve = (t[:k].detach().clone().requires_grad_() for t in (q_g, k_g, v_g))
    ge = g[:k].contiguous()
    with torch.no_grad():
        ref, res["eager_fwd_peak_bytes"] = peak(lambda: eager_expression(ve, qe, ke, radius), dev)
        res["max_abs_diff"] = float((out.vecs[:k] - ref).abs().max())
        del ref
        res["eager_fwd_us"], res["eager_fwd_spread_us"] = timed(lambda: eager_expression(ve, qe, ke, radius))

    def eager_fwd_bwd():
        qe.grad, ke.grad, ve.grad = None, None, None
        eager_expression(ve, qe, ke, radius).backward(ge)

    _, res["eager_fwd_bwd_peak_bytes"] = peak(eager_fwd_bwd, dev)
    res["eager_fwd_bwd_us"], res["eager_fwd_bwd_spread_us"] = timed(eager_fwd_bwd)
    for nm, fused_grad, t in zip(("d_query", "d_key", "d_flow"), d_fused, (qe, ke, ve)):
        res["max_abs_diff_" + nm] = float((fused_grad[:k] - t.grad).abs().max())
    for key_ in ("fwd", "fwd_bwd"):
        res["time_ratio_" + key_] = round((res[key_ + "_us"] / n) / (res["eager_" + key_ + "_us"] / k), 3)
        res["mem_ratio_" + key_] = round((res[key_ + "_peak_bytes"] / n) / (res["eager_" + key_ + "_peak_bytes"] / k), 6)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='all', choices=tuple(CASES) + ('all',))
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
    for name in (tuple(CASES) if a.case == 'all' else (a.case,)):
        res = {"op": "Flow.propagate", "features": "float32", "iters": a.iters, "warmup": a.warmup, "blocks": a.blocks}
        res.update(measure(name, a.batch, a.channels, a, dev))
        print(json.dumps(res), flush=True)
        done[name] = res
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(done, indent=1, sort_keys=True) + "\n")


if __name__ == '__main__':
    main()
