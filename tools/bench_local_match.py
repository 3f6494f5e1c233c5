#!/usr/bin/env python3
"""Flow.match_local next to the eager composition in fp32 torch, all in one process: `Flow.apply` of `other` (the warp),
GMFlow's window expression -- the unfold of the warped features, the correlation over sqrt(C), the positions outside the frame at -1e9,
the softmax, the expectation of the offsets -- and the add.

    python tools/bench_local_match.py [--case NAME|all] [--batch 8] [--channels 128] [--iters 3] [--warmup 1] [--blocks 5]
                                      [--out profiles/local_match_bench.json]

Cases: `r1` and `r4` at 270 x 480 (a 1080p frame at quarter resolution) with radius 1 and 4; B = 8 and C = 128 by default.  The features
are N(0, 1), float32, the vectors of a 't' flow N(0, 4), the upstream gradient uniform in [-1, 1), the flow's mask all True and
considered (the kernels read it).  Every figure is the median of `blocks` blocks of `iters` calls each, after `warmup` calls, by HIP
events; `*_spread_us` is the largest minus the smallest block.  Peak memory is torch.cuda.max_memory_allocated beyond what was allocated
before the call (the inputs).  The eager composition runs on the first `eager_images` images: the whole batch, or as many as leave its
intermediates (three unfolded tensors of 4 (2 r + 1)^2 C H W bytes an image) under half the device's free memory; the ratios compare per
image.  Prints one JSON line per case and with --out writes {case: result} (an existing file keeps its other cases):
  fwd_us, fwd_peak_bytes                     flow.match_local(feat, other, radius): one launch, the allocations, the Flow
  fwd_bwd_us, fwd_bwd_peak_bytes             ... and .vecs.backward(g) with feat, other and the vectors requiring a gradient
  fwd_tflops                                 2 C (2 r + 1)^2 flops a pixel over fwd_us
  eager_fwd_us, eager_fwd_peak_bytes, ...    the eager composition on `eager_images` images, and its forward plus backward
  time_ratio_fwd, time_ratio_fwd_bwd         fused over eager, per image;  mem_ratio_fwd, mem_ratio_fwd_bwd likewise (peak bytes)
  max_abs_diff*                              the largest differences between the two results over the INTERIOR pixels: those whose whole
                                             window is usable (the two differ by definition where a sample leaves the frame: Flow.apply
                                             keeps the part of a sample that lies inside, W' is +0 there); `interior_fraction` of all
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import oflibpytorch_amd as ofl  # noqa: E402

CASES = {"r1": (270, 480, 1), "r4": (270, 480, 4)}


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


def eager_expression(vecs, feat, other, radius):
    """GMFlow's local correlation, softmax and flow update of a 't' flow, on the features warped by Flow.apply"""
    n, c, h, w = feat.shape
    warped = ofl.Flow(vecs, 't').apply(other)
    k = 2 * radius + 1
    win = torch.nn.functional.unfold(warped, k, padding=radius).view(n, c, k * k, h * w)
    corr = (feat.view(n, c, 1, h * w) * win).sum(1) / (c ** 0.5)
    inside = torch.nn.functional.unfold(torch.ones((1, 1, h, w), device=feat.device), k, padding=radius).view(1, k * k, h * w) > 0
    prob = torch.softmax(corr.masked_fill(~inside, -1e9), dim=1)
    r = torch.arange(-radius, radius + 1, device=feat.device, dtype=feat.dtype)
    offs = torch.stack([r.repeat(k), r.repeat_interleave(k)], 0)                             # [2, D]: dx innermost, dy outermost
    return vecs - torch.einsum('kd,ndp->nkp', offs, prob).view(n, 2, h, w)


def peak(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated(dev) - base


def interior_of(vecs, radius):
    """bool [n,1,h,w]: the pixels whose whole window lies in the frame and samples inside it ('t' flow: the sample position is p - a)"""
    n, _, h, w = vecs.shape
    yy, xx = torch.meshgrid(torch.arange(h, device=vecs.device), torch.arange(w, device=vecs.device), indexing='ij')
    px, py = xx[None] - vecs[:, 0], yy[None] - vecs[:, 1]
    ok = ((px >= 0) & (px <= w - 1) & (py >= 0) & (py <= h - 1))[:, None].float()
    k = 2 * radius + 1
    return torch.nn.functional.avg_pool2d(ok, k, stride=1, padding=radius, count_include_pad=True) > 1.0 - 0.5 / (k * k)


def measure(name, n, c, a, dev):
    h, w, radius = CASES[name]
    gen = torch.Generator(device=dev).manual_seed(13)
    feat = torch.randn((n, c, h, w), device=dev, generator=gen)
    other = torch.randn((n, c, h, w), device=dev, generator=gen)
    vecs = torch.randn((n, 2, h, w), device=dev, generator=gen) * 2
    g = torch.rand((n, 2, h, w), device=dev, generator=gen) * 2 - 1
    timed = lambda fn: events(fn, a.iters, a.warmup, a.blocks)
    d = (2 * radius + 1) ** 2
    inter = 4 * d * c * h * w
    res = {"case": name, "batch": n, "channels": c, "h": h, "w": w, "radius": radius, "eager_intermediate_bytes_per_image": inter}
    flow = ofl.Flow(vecs, 't')
    fused = lambda: flow.match_local(feat, other, radius)
    out, res["fwd_peak_bytes"] = peak(fused, dev)
    res["fwd_us"], res["fwd_spread_us"] = timed(fused)
    res["fwd_tflops"] = round(2.0 * c * d * h * w * n / res["fwd_us"] / 1e6, 2)
    f_g, o_g, v_g = feat.clone().requires_grad_(), other.clone().requires_grad_(), vecs.clone().requires_grad_()

    def fused_fwd_bwd():
        f_g.grad, o_g.grad, v_g.grad = None, None, None
        ofl.Flow(v_g, 't').match_local(f_g, o_g, radius).vecs.backward(g)

    _, res["fwd_bwd_peak_bytes"] = peak(fused_fwd_bwd, dev)
    res["fwd_bwd_us"], res["fwd_bwd_spread_us"] = timed(fused_fwd_bwd)
    f_g.grad, o_g.grad, v_g.grad = None, None, None
    # the eager composition, on as many images as fit
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info(dev)[0]
    k = max(1, min(n, int(free // 2 // (3 * inter))))
    res["device_free_bytes"], res["eager_images"] = int(free), k
    fe, oe, ve = (t[:k].detach().clone().requires_grad_() for t in (f_g, o_g, v_g))
    ge = g[:k].contiguous()
    inner = interior_of(vecs[:k], radius)
    res["interior_fraction"] = round(float(inner.float().mean()), 4)
    with torch.no_grad():
        ref, res["eager_fwd_peak_bytes"] = peak(lambda: eager_expression(ve, fe, oe, radius), dev)
        res["max_abs_diff"] = float(((out.vecs[:k] - ref).abs() * inner).max())
        del ref
        res["eager_fwd_us"], res["eager_fwd_spread_us"] = timed(lambda: eager_expression(ve, fe, oe, radius))

    def eager_fwd_bwd():
        fe.grad, oe.grad, ve.grad = None, None, None
        eager_expression(ve, fe, oe, radius).backward(ge * inner)

    _, res["eager_fwd_bwd_peak_bytes"] = peak(eager_fwd_bwd, dev)
    res["eager_fwd_bwd_us"], res["eager_fwd_bwd_spread_us"] = timed(eager_fwd_bwd)
    # the gradients are compared under an upstream gradient that is zero outside the interior, where the two definitions agree
    f2, o2, v2 = (t[:k].detach().clone().requires_grad_() for t in (f_g, o_g, v_g))
    ofl.Flow(v2, 't').match_local(f2, o2, radius).vecs.backward(ge * inner)
    for nm, fused_grad, t in zip(("d_feat", "d_other", "d_flow"), (f2.grad, o2.grad, v2.grad), (fe, oe, ve)):
        res["max_abs_diff_" + nm] = float((fused_grad - t.grad).abs().max())
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
        res = {"op": "Flow.match_local", "features": "float32", "iters": a.iters, "warmup": a.warmup, "blocks": a.blocks}
        res.update(measure(name, a.batch, a.channels, a, dev))
        print(json.dumps(res), flush=True)
        done[name] = res
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(done, indent=1, sort_keys=True) + "\n")


if __name__ == '__main__':
    main()
