#!/usr/bin/env python3
"""Flow.chain on a clip of 1080p flows, next to the Python fold of combine_with(..., 3) on the same flow objects and to
a device copy of the bytes the chain cannot avoid, all in one process.

    python tools/bench_chain.py [--batch 16] [--t 8] [--iters 10] [--blocks 5] [--warmup 3] [--out profiles/chain_bench.json]

T 's' flows of 1080 x 1920 in fp32, each the sigma-8 flow of bench.py (another seed per frame) divided by sqrt(T), so that the accumulated
displacement stays of that flow's order; every flow has a mask with 20 % holes in cells of 16 x 16 pixels.  The flow objects are made
ahead and their flag words are known, as after any earlier use.  The chain moves at least T * 9 + 9 B/px: every flow's vectors and mask
byte once, the result's vectors and mask once.  Times by HIP events: the median of `--blocks` blocks of `--iters` calls after a warm-up,
with the spread (max - min) / median; the blocks of the three calls alternate.  Prints (and with --out writes) one JSON line:
  chain_us, chain_gbs        Flow.chain(flows): one launch and two allocations; GB/s on the (9 T + 9) B/px
  chain_all_us               Flow.chain(flows, return_all=True): the same walk storing all T - 1 partial chains
  fold_us                    acc = flows[0]; acc = acc.combine_with(f, 3) for the others: T - 1 launches, each result wrapped and validated
  copy_us, copy_gbs          dst.copy_(src) of as many bytes in all (half read, half written)
  chain_vs_copy              chain_gbs / copy_gbs
  fold_vs_chain              fold_us / chain_us (above 1: the chain is faster)
  chain_peak_bytes, fold_peak_bytes, chain_all_peak_bytes     peak device memory of one call beyond what was allocated before it
  same_bits                  the chain and the fold give the same vectors and mask, bit for bit (asserted once, outside the timed region)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import oflibpytorch_amd as ofl  # noqa: E402
from oflibpytorch_amd import _native  # noqa: E402


def events(fns, iters, blocks, warmup):
    """Per function of `fns`: (median microseconds per call over `blocks` blocks of `iters` calls, (max - min) / median).  The blocks
    of the functions alternate, so that a drift of the machine meets all of them alike."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    times = [[] for _ in fns]
    for _ in range(blocks):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) / iters * 1e3)
    meds = [statistics.median(ts) for ts in times]
    return [(med, (max(ts) - min(ts)) / med) for med, ts in zip(meds, times)]


def peak_of(fn):
    """Peak device memory of one call beyond what was allocated before it, in bytes (the result is alive at the peak)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def fold(flows):
    acc = flows[0]
    for f in flows[1:]:
        acc = acc.combine_with(f, 3)
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--t', type=int, default=8)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    n, t, h, w = a.batch, a.t, a.height, a.width
    gen = torch.Generator(device='cpu').manual_seed(11)
    flows = []
    for k in range(t):
        vecs = bench.smooth_flow(n, h, w, 8.0, 3000 + k, dev) / (t ** 0.5)
        cells = (torch.rand(n, (h + 15) // 16, (w + 15) // 16, generator=gen) > 0.2).to(dev)
        mask = cells.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :h, :w].contiguous()
        f = ofl.Flow(vecs, 's', mask)
        f._flags()                                             # (known, as after any earlier use of the flow)
        flows.append(f)
    px = n * h * w
    nbytes = (9 * t + 9) * px
    res = {"op": "flow_chain", "batch": n, "t": t, "h": h, "w": w, "ref": "s", "iters": a.iters, "blocks": a.blocks, "bytes": nbytes}

    one = ofl.Flow.chain(flows)
    res["kernel"] = _native.last_kernel_name()
    ref = fold(flows)
    same = bool(torch.equal(one.vecs.view(torch.int32), ref.vecs.view(torch.int32))) and bool(torch.equal(one.mask, ref.mask))
    res["same_bits"] = same
    res["valid_share"] = round(float(one.mask.float().mean()), 4)
    res["max_displacement_px"] = round(float(one.vecs.abs().max()), 2)
    assert same, "Flow.chain and the fold of combine_with(..., 3) differ"
    every = ofl.Flow.chain(flows, return_all=True)
    assert bool(torch.equal(every[-1].vecs.view(torch.int32), one.vecs.view(torch.int32))) and bool(torch.equal(every[-1].mask, one.mask))
    del one, ref, every

    res["chain_peak_bytes"] = peak_of(lambda: ofl.Flow.chain(flows))
    res["chain_all_peak_bytes"] = peak_of(lambda: ofl.Flow.chain(flows, return_all=True))
    res["fold_peak_bytes"] = peak_of(lambda: fold(flows))

    timed = events([lambda: ofl.Flow.chain(flows), lambda: fold(flows), lambda: ofl.Flow.chain(flows, return_all=True)],
                   a.iters, a.blocks, a.warmup)
    us, spread = timed[0]
    res["chain_us"], res["chain_spread"], res["chain_gbs"] = round(us, 1), round(spread, 3), round(nbytes / us / 1e3, 1)
    us, spread = timed[1]
    res["fold_us"], res["fold_spread"] = round(us, 1), round(spread, 3)
    us, spread = timed[2]
    res["chain_all_us"], res["chain_all_spread"] = round(us, 1), round(spread, 3)
    res["chain_all_gbs"] = round((9 * t + 9 * (t - 1)) * px / us / 1e3, 1)
    torch.cuda.empty_cache()
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    us, spread = events([lambda: dst.copy_(src)], a.iters, a.blocks, a.warmup)[0]
    res["copy_us"], res["copy_spread"], res["copy_gbs"] = round(us, 1), round(spread, 3), round(2 * (nbytes // 2) / us / 1e3, 1)
    res["chain_vs_copy"] = round(res["chain_gbs"] / res["copy_gbs"], 3)
    res["fold_vs_chain"] = round(res["fold_us"] / res["chain_us"], 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + "\n")


if __name__ == '__main__':
    main()
