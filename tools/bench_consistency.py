#!/usr/bin/env python3
"""Flow.consistency on a batch of 1080p frames, next to the expression a user writes without it -- combine_with(mode 3)
followed by torch operations -- and to a device copy of as many bytes as the fused call has to move, all in one process.

    python tools/bench_consistency.py [--batch 64] [--h 1080] [--w 1920] [--iters 50] [--warmup 5] [--out profiles/consistency_bench.json]

`a` is the bench's smooth flow (sigma 8, bench.smooth_flow) as an 's' flow, `back` its inverse resampled at its target (a.invert()) with
uniform noise of +-2 px on a quarter of the frame; both masks have 20 % holes.  Times by HIP events.  Prints (and with --out writes) one
JSON line:
  fused_us, fused_gbs       Flow.consistency(back): both kernels, the allocations and the torch divisions of the record; GB/s on the
                            24 B/px the call cannot avoid (8 + 8 + 1 + 1 read, 4 + 1 + 1 written; the gather's re-reads are not counted)
  mask_us                   Flow.consistency_mask(back): the same pass with one byte map written and no record
  composed_us               a.combine_with(back, 3), then the torch operations that give the same three maps and five numbers per image
  mode3_us                  the combine_with(back, 3) of that expression alone
  copy_us, copy_gbs         dst.copy_(src) of 24 B/px in all (half read, half written)
  fused_vs_copy             fused_gbs / copy_gbs
  composed_vs_fused         composed_us / fused_us
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import oflibpytorch_amd as ofl  # noqa: E402
from oflibpytorch_amd import _native  # noqa: E402

ALPHA, BETA = 0.01, 0.5


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


def composed(a, back):
    """What Flow.consistency returns, from the composed flow and eager torch."""
    c = a.combine_with(back, 3)
    known, v, av = c.mask, c.vecs, a.vecs
    e2 = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]
    e = e2.sqrt()
    p = v - av                                       # the partner
    m2 = (av[:, 0] * av[:, 0] + av[:, 1] * av[:, 1]) + (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1])
    cons = known & (e2 <= ALPHA * m2 + BETA)
    err = torch.where(known, e, torch.zeros_like(e))
    count, ccount = known.sum((1, 2)), cons.sum((1, 2))
    total = err.sum((1, 2), dtype=torch.float64)
    ctotal = torch.where(cons, e, torch.zeros_like(e)).sum((1, 2), dtype=torch.float64)
    return {'error': err, 'consistent': cons, 'known': known, 'count': count, 'consistent_count': ccount, 'rate': ccount / count,
            'mean_error': total / count, 'max_error': err.amax((1, 2)).double(), 'mean_error_consistent': ctotal / ccount}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--h', type=int, default=1080)
    ap.add_argument('--w', type=int, default=1920)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    n, h, w = args.batch, args.h, args.w
    gen = torch.Generator(device=dev).manual_seed(11)
    am = torch.rand((n, h, w), device=dev, generator=gen) > 0.2
    bm = torch.rand((n, h, w), device=dev, generator=gen) > 0.2
    a = ofl.Flow(bench.smooth_flow(n, h, w, 8.0, 1000, dev), 's', am)
    inv = ofl.Flow(a.vecs, 's').invert()             # -a resampled at its target (every source pixel takes part)
    bv = inv.vecs.clone()
    del inv
    bv[:, :, h // 2:, w // 2:] += torch.rand((n, 2, h - h // 2, w - w // 2), device=dev, generator=gen) * 4.0 - 2.0
    back = ofl.Flow(bv, 's', bm)
    px = n * h * w
    res = {"op": "Flow.consistency", "batch": n, "h": h, "w": w, "iters": args.iters, "alpha": ALPHA, "beta": BETA,
           "min_bytes_per_call": 24 * px}

    got = a.consistency(back)
    res["kernel"] = _native.last_kernel_name()
    want = composed(a, back)
    res["known_agree"] = bool(torch.equal(got['known'], want['known']))
    res["consistent_agree"] = bool(torch.equal(got['consistent'], want['consistent']))
    res["error_bits_agree"] = bool(torch.equal(got['error'].view(torch.int32), want['error'].view(torch.int32)))
    res["counts_agree"] = bool(torch.equal(got['count'], want['count']) and torch.equal(got['consistent_count'], want['consistent_count']))
    res["known_share"] = round(float(got['count'].sum()) / px, 4)
    res["consistent_share"] = round(float(got['consistent_count'].sum()) / px, 4)
    res["mean_error_fused"] = float((got['mean_error'] * got['count']).sum() / got['count'].sum())
    res["mean_error_composed"] = float((want['mean_error'] * want['count']).sum() / want['count'].sum())
    del got, want

    res["fused_us"] = round(events(lambda: a.consistency(back), args.iters, args.warmup), 1)
    res["fused_gbs"] = round(24 * px / res["fused_us"] / 1e3, 1)
    res["mask_us"] = round(events(lambda: a.consistency_mask(back), args.iters, args.warmup), 1)
    res["composed_us"] = round(events(lambda: composed(a, back), args.iters, args.warmup), 1)
    res["mode3_us"] = round(events(lambda: a.combine_with(back, 3), args.iters, args.warmup), 1)
    src = torch.empty(12 * px, dtype=torch.uint8, device=dev)
    dst = torch.empty(12 * px, dtype=torch.uint8, device=dev)
    res["copy_us"] = round(events(lambda: dst.copy_(src), args.iters, args.warmup), 1)
    res["copy_gbs"] = round(24 * px / res["copy_us"] / 1e3, 1)
    res["fused_vs_copy"] = round(res["fused_gbs"] / res["copy_gbs"], 3)
    res["composed_vs_fused"] = round(res["composed_us"] / res["fused_us"], 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + "\n")


if __name__ == '__main__':
    main()
