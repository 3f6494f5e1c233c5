#!/usr/bin/env python3
"""Flow.sequence_loss on a batch of training crops and of 1080p frames, next to RAFT's eager loop on the same tensors and
to a device copy of as many bytes, all in one process.

    python tools/bench_sequence_loss.py [--batch 8] [--t 12] [--iters 20] [--blocks 5] [--warmup 5] [--out profiles/sequence_loss_bench.json]

Per frame size (368 x 768 and 1080 x 1920): T fp32 predictions that approach a smooth ground truth, a mask with 20 % holes.  The forward
reads (8 T + 9) B/px (T predictions, the ground truth, the mask); the forward and backward with all T gradients read that twice and write
8 T B/px.  Times by HIP events: the median of `--blocks` blocks of `--iters` calls after a warm-up, with the spread (max - min) / median.
Prints (and with --out writes) one JSON line, per size:
  fwd_us, fwd_gbs             Flow.sequence_loss(flows, gt) on flow objects made ahead, without a gradient: both launches, the allocations,
                              the torch operations that form the loss; GB/s on the (8 T + 9) B/px
  wrapper_fwd_us              flow_sequence_loss(stack, gt, mask) on the tensors: the same and the validation of the ground truth
  fwd_bwd_us, fwd_bwd_gbs     Flow.sequence_loss with the stack requiring a gradient, .sum().backward(): GB/s on (24 T + 18) B/px
  eager_fwd_us, eager_fwd_bwd_us   RAFT's loop (train.py) in eager torch on the same tensors
  copy_us, copy_gbs           dst.copy_(src) of as many bytes in all (half read, half written) as the forward reads
  fwd_vs_copy                 fwd_gbs / copy_gbs
  fwd_vs_eager, fwd_bwd_vs_eager   eager time / fused time
  loss_new, loss_eager        the two scalars (they differ by fp32 rounding of the eager means)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import oflibpytorch_amd as ofl  # noqa: E402
from oflibpytorch_amd import _native  # noqa: E402


def events(fn, iters, blocks, warmup):
    """(median microseconds per call over `blocks` blocks of `iters` calls, (max - min) / median)"""
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
    med = statistics.median(times)
    return med, (max(times) - min(times)) / med


def raft_loop(preds, gt, valid, gamma=0.8, max_flow=400.0):
    """RAFT's sequence_loss (train.py), the loss only"""
    n_predictions = len(preds)
    flow_loss = 0.0
    mag = torch.sum(gt ** 2, dim=1).sqrt()
    valid = (valid >= 0.5) & (mag < max_flow)
    for i in range(n_predictions):
        i_weight = gamma ** (n_predictions - i - 1)
        i_loss = (preds[i] - gt).abs()
        flow_loss += i_weight * (valid[:, None] * i_loss).mean()
    return flow_loss


def one_size(n, t, h, w, a, dev):
    gen = torch.Generator(device=dev).manual_seed(5)
    yy, xx = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing='ij')
    speed = 30.0 * (xx / (w - 1) + yy / (h - 1))
    gt = torch.empty((n, 2, h, w), device=dev)
    for i in range(n):
        theta = 6.2831853 * (yy / h + 0.37 * i)
        gt[i, 0], gt[i, 1] = speed * torch.cos(theta), speed * torch.sin(theta)
    stack = torch.empty((t, n, 2, h, w), device=dev)
    for i in range(t):
        stack[i] = gt + torch.randn((n, 2, h, w), device=dev, generator=gen) * (2.5 * (t - i) / t)
    mask = torch.rand((n, h, w), device=dev, generator=gen) > 0.2
    valid = mask.float()
    px = n * h * w
    fwd_bytes, both_bytes = (8 * t + 9) * px, (24 * t + 18) * px
    res = {"h": h, "w": w, "bytes_read_fwd": fwd_bytes}

    flows, truth = [ofl.Flow(p, 't') for p in stack.unbind(0)], ofl.Flow(gt, 't', mask)
    res["loss_new"] = float(ofl.Flow.sequence_loss(flows, truth).mean())
    res["kernel"] = _native.last_kernel_name()
    res["loss_eager"] = float(raft_loop(list(stack.unbind(0)), gt, valid))

    us, spread = events(lambda: ofl.Flow.sequence_loss(flows, truth), a.iters, a.blocks, a.warmup)
    res["fwd_us"], res["fwd_spread"], res["fwd_gbs"] = round(us, 1), round(spread, 3), round(fwd_bytes / us / 1e3, 1)
    us, spread = events(lambda: ofl.flow_sequence_loss(stack, gt, mask), a.iters, a.blocks, a.warmup)
    res["wrapper_fwd_us"], res["wrapper_fwd_spread"] = round(us, 1), round(spread, 3)
    us, spread = events(lambda: raft_loop(list(stack.unbind(0)), gt, valid), a.iters, a.blocks, a.warmup)
    res["eager_fwd_us"], res["eager_fwd_spread"] = round(us, 1), round(spread, 3)

    leaf = stack.clone().requires_grad_()
    flows_g = [ofl.Flow(p, 't') for p in leaf.unbind(0)]

    def new_fwd_bwd():
        leaf.grad = None
        ofl.Flow.sequence_loss(flows_g, truth).sum().backward()

    def eager_fwd_bwd():
        leaf.grad = None
        raft_loop(list(leaf.unbind(0)), gt, valid).backward()

    us, spread = events(new_fwd_bwd, a.iters, a.blocks, a.warmup)
    res["fwd_bwd_us"], res["fwd_bwd_spread"], res["fwd_bwd_gbs"] = round(us, 1), round(spread, 3), round(both_bytes / us / 1e3, 1)
    res["grad_kernel"] = _native.last_kernel_name()
    us, spread = events(eager_fwd_bwd, a.iters, a.blocks, a.warmup)
    res["eager_fwd_bwd_us"], res["eager_fwd_bwd_spread"] = round(us, 1), round(spread, 3)
    leaf.grad = None
    del leaf, flows_g

    src = torch.empty(fwd_bytes // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty(fwd_bytes // 2, dtype=torch.uint8, device=dev)
    us, spread = events(lambda: dst.copy_(src), a.iters, a.blocks, a.warmup)
    res["copy_us"], res["copy_spread"], res["copy_gbs"] = round(us, 1), round(spread, 3), round(2 * (fwd_bytes // 2) / us / 1e3, 1)
    res["fwd_vs_copy"] = round(res["fwd_gbs"] / res["copy_gbs"], 3)
    res["fwd_vs_eager"] = round(res["eager_fwd_us"] / res["fwd_us"], 1)
    res["fwd_bwd_vs_eager"] = round(res["eager_fwd_bwd_us"] / res["fwd_bwd_us"], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--t', type=int, default=12)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--sizes', default="368x768,1080x1920")
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    res = {"op": "flow_sequence_loss", "batch": a.batch, "t": a.t, "iters": a.iters, "blocks": a.blocks, "sizes": []}
    for size in a.sizes.split(","):
        h, w = (int(v) for v in size.split("x"))
        res["sizes"].append(one_size(a.batch, a.t, h, w, a, dev))
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + "\n")


if __name__ == '__main__':
    main()
