#!/usr/bin/env python3
"""Flow.error_stats and Flow.epe on a batch of 1080p frames, next to the torch expression a user writes today and to a
device copy of as many bytes, all in one process.

    python tools/bench_metrics.py [--batch 64] [--h 1080] [--w 1920] [--iters 50] [--warmup 5] [--out profiles/metrics_bench.json]

The ground truth is a smooth flow, the estimate adds noise of sigma 2.5, both masks have 20 % holes.  At the default size one call reads
2.4 GB (two fp32 flows, two masks: 18 B/px), several times the last-level cache, so nothing rotates.  Times by HIP events.  Prints (and with
--out writes) one JSON line:
  stats_us, stats_gbs       Flow.error_stats(gt): both kernels, the allocations and the torch divisions of the record; GB/s on the 18 B/px
  map_us                    Flow.epe_map(gt): the same pass with the 4 B/px map written
  epe_fwd_us                Flow.epe(gt) without a gradient
  epe_fwd_bwd_us, _gbs      Flow.epe(gt).sum().backward() with the estimate requiring a gradient: 18 B/px read twice, 8 B/px written
  torch_stats_us            the same numbers (mean, 1 / 3 / 5 px rates, Fl, three speed bins) from torch expressions over the whole batch
  torch_fwd_bwd_us          the masked mean of torch.linalg.vector_norm(est - gt, dim=1) per image, forward and backward
  copy_us, copy_gbs         dst.copy_(src) of as many bytes in all (half read, half written) as error_stats reads
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


def torch_stats(est, gt, em, gm):
    d = est - gt
    e = (d * d).sum(1).sqrt()
    g = (gt * gt).sum(1).sqrt()
    valid = em & gm
    ev, gv = e[valid], g[valid]
    out = [ev.mean(), ev.max()] + [(ev > t).float().mean() for t in (1.0, 3.0, 5.0)] + [((ev > 3.0) & (ev > 0.05 * gv)).float().mean()]
    for sel in (gv < 10, (gv >= 10) & (gv < 40), gv >= 40):
        out.append(ev[sel].mean())
    return torch.stack(out)


def torch_loss(est, gt, em, gm):
    valid = (em & gm).float()
    e = torch.linalg.vector_norm(est - gt, dim=1)
    return ((e * valid).sum((1, 2)) / valid.sum((1, 2))).sum()


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
    n, h, w = a.batch, a.h, a.w
    gen = torch.Generator(device=dev).manual_seed(5)
    yy, xx = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing='ij')
    speed = 30.0 * (xx / (w - 1) + yy / (h - 1))
    gt_v = torch.empty((n, 2, h, w), device=dev)
    for i in range(n):
        theta = 6.2831853 * (yy / h + 0.37 * i)
        gt_v[i, 0], gt_v[i, 1] = speed * torch.cos(theta), speed * torch.sin(theta)
    est_v = gt_v + torch.randn((n, 2, h, w), device=dev, generator=gen) * 2.5
    em = torch.rand((n, h, w), device=dev, generator=gen) > 0.2
    gm = torch.rand((n, h, w), device=dev, generator=gen) > 0.2
    est, gt = ofl.Flow(est_v, 't', em), ofl.Flow(gt_v, 't', gm)
    px = n * h * w
    res = {"op": "Flow.error_stats / Flow.epe", "batch": n, "h": h, "w": w, "iters": a.iters, "bytes_read_per_call": 18 * px}

    s = est.error_stats(gt)
    res["kernel"] = _native.last_kernel_name()
    want = torch_stats(est_v, gt_v, em, gm)
    valid = em & gm
    res["mean_epe_new"] = float((s['epe'] * s['count']).sum() / s['count'].sum())
    res["mean_epe_torch"] = float(want[0])
    res["counts_agree"] = bool(torch.equal(s['count'], valid.sum((1, 2))))
    del want, valid

    res["stats_us"] = round(events(lambda: est.error_stats(gt), a.iters, a.warmup), 1)
    res["stats_gbs"] = round(18 * px / res["stats_us"] / 1e3, 1)
    res["map_us"] = round(events(lambda: est.epe_map(gt), a.iters, a.warmup), 1)
    res["epe_fwd_us"] = round(events(lambda: est.epe(gt), a.iters, a.warmup), 1)

    leaf = est_v.clone().requires_grad_()
    est_g = ofl.Flow(leaf, 't', em)

    def new_fwd_bwd():
        leaf.grad = None
        est_g.epe(gt).sum().backward()

    res["epe_fwd_bwd_us"] = round(events(new_fwd_bwd, a.iters, a.warmup), 1)
    res["epe_fwd_bwd_gbs"] = round((18 + 18 + 8) * px / res["epe_fwd_bwd_us"] / 1e3, 1)
    res["grad_kernel"] = _native.last_kernel_name()

    def torch_fwd_bwd():
        leaf.grad = None
        torch_loss(leaf, gt_v, em, gm).backward()

    res["torch_stats_us"] = round(events(lambda: torch_stats(est_v, gt_v, em, gm), a.iters, a.warmup), 1)
    res["torch_fwd_bwd_us"] = round(events(torch_fwd_bwd, a.iters, a.warmup), 1)
    leaf.grad = None

    src = torch.empty(9 * px, dtype=torch.uint8, device=dev)
    dst = torch.empty(9 * px, dtype=torch.uint8, device=dev)
    res["copy_us"] = round(events(lambda: dst.copy_(src), a.iters, a.warmup), 1)
    res["copy_gbs"] = round(18 * px / res["copy_us"] / 1e3, 1)
    res["stats_vs_copy"] = round(res["stats_gbs"] / res["copy_gbs"], 3)
    res["stats_vs_torch"] = round(res["torch_stats_us"] / res["stats_us"], 1)
    res["fwd_bwd_vs_torch"] = round(res["torch_fwd_bwd_us"] / res["epe_fwd_bwd_us"], 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + "\n")


if __name__ == '__main__':
    main()
