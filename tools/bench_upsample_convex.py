#!/usr/bin/env python3
"""Flow.upsample_convex on a batch of eighth-resolution 1080p flows, next to RAFT's eager expression in fp32 torch
(softmax / unfold / multiply / sum / permute) and to a device copy of as many bytes as the forward must move, all in one process.

    python tools/bench_upsample_convex.py [--batch 8] [--h 135] [--w 240] [--iters 3] [--warmup 1] [--blocks 5]
                                          [--out profiles/upsample_convex_bench.json]

The flow is bench.py's smooth flow of sigma 8 scaled by 1/8, its mask has 20 % holes, the logits are N(0, 1), float32.  The algorithmic
bytes of the forward are 8 (flow) + 1 (mask) + 36 k^2 (logits) read and 8 k^2 (vectors) + k^2 (mask) written per coarse pixel.  Every
figure is the median of `blocks` blocks of `iters` calls each, after `warmup` calls, by HIP events; `*_spread_us` is the largest minus the
smallest block.  Prints (and with --out writes) one JSON line:
  fwd_us, fwd_gbs, fwd_peak_bytes            Flow.upsample_convex(logits) at k = 8: one launch, the allocations and the result's Flow
  fwd_bwd_us, fwd_bwd_peak_bytes             ... and .backward(g) with the logits and the vectors requiring a gradient
  copy_us, copy_gbs, fwd_vs_copy             dst.copy_(src) of as many bytes in all as the forward reads and writes
  eager_fwd_us, eager_fwd_peak_bytes         RAFT's expression on the same tensors (vectors only: it makes no mask)
  eager_fwd_bwd_us, eager_fwd_bwd_peak_bytes ... and its backward into the logits and the vectors
  max_abs_diff                               the largest difference between the two results
  fwd_wins, fwd_bwd_wins                     the fused median lies below the eager median by more than the sum of the two spreads
  k4, k2                                     the forward alone at k = 4 (2 h x 2 w coarse) and k = 2 (4 h x 4 w): fwd_us, eager_fwd_us, ...
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
from oflibpytorch_amd import _native, _upsample  # noqa: E402


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


def raft_expression(flow, logits, k):
    """RAFT's upsample_flow"""
    n, _, h, w = flow.shape
    mask = torch.softmax(logits.view(n, 1, 9, k, k, h, w), dim=2)
    up = torch.nn.functional.unfold(k * flow, [3, 3], padding=1).view(n, 2, 9, 1, 1, h, w)
    return torch.sum(mask * up, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(n, 2, k * h, k * w)


def peak(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated(dev) - base


def measure(n, h, w, k, a, dev, backward):
    gen = torch.Generator(device=dev).manual_seed(5 + k)
    vecs = (smooth_flow(n, h, w, 8.0, 1000, dev) * 0.125).contiguous()
    mask = torch.rand((n, h, w), device=dev, generator=gen) > 0.2
    logits = torch.randn((n, 9 * k * k, h, w), device=dev, generator=gen)
    flow = ofl.Flow(vecs, 's', mask)
    timed = lambda fn: events(fn, a.iters, a.warmup, a.blocks)
    res = {"factor": k, "h": h, "w": w}
    nbytes = (8 + 1 + 36 * k * k + 9 * k * k) * n * h * w
    res["bytes_per_call"] = nbytes
    _upsample.flow_upsample_convex(vecs, mask, logits, k)
    res["kernel"] = _native.last_kernel_name()
    up, res["fwd_peak_bytes"] = peak(lambda: flow.upsample_convex(logits), dev)
    res["fwd_us"], res["fwd_spread_us"] = timed(lambda: flow.upsample_convex(logits))
    res["fwd_gbs"] = round(nbytes / res["fwd_us"] / 1e3, 1)
    with torch.no_grad():
        ref, res["eager_fwd_peak_bytes"] = peak(lambda: raft_expression(vecs, logits, k), dev)
        res["max_abs_diff"] = float((up.vecs - ref).abs().max())
        del ref
        res["eager_fwd_us"], res["eager_fwd_spread_us"] = timed(lambda: raft_expression(vecs, logits, k))
    del up
    res["fwd_wins"] = bool(res["fwd_us"] + res["fwd_spread_us"] + res["eager_fwd_spread_us"] < res["eager_fwd_us"])
    if backward:
        g = torch.rand((n, 2, k * h, k * w), device=dev, generator=gen) * 2 - 1
        v_g, l_g = vecs.clone().requires_grad_(), logits.clone().requires_grad_()
        flow_g = ofl.Flow(v_g, 's', mask)

        def fused_fwd_bwd():
            v_g.grad, l_g.grad = None, None
            flow_g.upsample_convex(l_g).vecs.backward(g)

        def eager_fwd_bwd():
            v_g.grad, l_g.grad = None, None
            raft_expression(v_g, l_g, k).backward(g)

        _, res["fwd_bwd_peak_bytes"] = peak(fused_fwd_bwd, dev)
        res["fwd_bwd_us"], res["fwd_bwd_spread_us"] = timed(fused_fwd_bwd)
        fused = (l_g.grad.clone(), v_g.grad.clone())
        _, res["eager_fwd_bwd_peak_bytes"] = peak(eager_fwd_bwd, dev)
        res["eager_fwd_bwd_us"], res["eager_fwd_bwd_spread_us"] = timed(eager_fwd_bwd)
        res["max_abs_diff_d_logits"] = float((fused[0] - l_g.grad).abs().max())
        res["max_abs_diff_d_vecs"] = float((fused[1] - v_g.grad).abs().max())
        res["fwd_bwd_wins"] = bool(res["fwd_bwd_us"] + res["fwd_bwd_spread_us"] + res["eager_fwd_bwd_spread_us"] < res["eager_fwd_bwd_us"])
        v_g.grad, l_g.grad = None, None
        del fused, g, v_g, l_g, flow_g
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        res["copy_us"], res["copy_spread_us"] = timed(lambda: dst.copy_(src))
        res["copy_gbs"] = round(2 * (nbytes // 2) / res["copy_us"] / 1e3, 1)
        res["fwd_vs_copy"] = round(res["fwd_gbs"] / res["copy_gbs"], 4)
        del src, dst
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--h', type=int, default=135)
    ap.add_argument('--w', type=int, default=240)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    res = {"op": "Flow.upsample_convex", "batch": a.batch, "logits": "float32", "ref": "s", "sigma": 8, "flow_scale": 0.125,
           "iters": a.iters, "warmup": a.warmup, "blocks": a.blocks}
    res.update(measure(a.batch, a.h, a.w, 8, a, dev, True))
    print(json.dumps(res), file=sys.stderr, flush=True)
    res["k4"] = measure(a.batch, 2 * a.h, 2 * a.w, 4, a, dev, False)
    res["k2"] = measure(a.batch, 4 * a.h, 4 * a.w, 2, a, dev, False)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + "\n")


if __name__ == '__main__':
    main()
