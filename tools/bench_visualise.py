#!/usr/bin/env python3
"""Flow.visualise on the device: B = 64 1080p fp32 flows, timed by HIP events over many calls after warm-up.

    python tools/bench_visualise.py [--batch 64] [--h 1080] [--w 1920] [--iters 100] [--warmup 10] [--oracle-batch 2]
                                    [--only default|given|hsv]

Prints one JSON line: ms per call of visualise('bgr') as a device tensor with the default range_max (the per-image 99th
percentile: three histogram passes over the flow + the colour pass) and with a given range_max (the colour pass only), and of
visualise('hsv') (a NumPy array, so its time includes the copy to the host); the bytes each moves (computed from the shapes)
and their share of 8 TB/s; and the NumPy oracle's time at a small batch (the reference's host computation, for scale).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import oflibpytorch_amd as ofl  # noqa: E402

PEAK = 8e12


def smooth(n, h, w, seed, dev):
    g = torch.Generator().manual_seed(seed)
    lo = torch.randn(n, 2, 6, 9, generator=g) * 12
    out = torch.empty(n, 2, h, w, device=dev)
    for i in range(0, n, 8):                                 # (bicubic upsampling in pieces: bounded temporaries)
        out[i:i + 8] = torch.nn.functional.interpolate(lo[i:i + 8].to(dev), size=(h, w), mode='bicubic', align_corners=True)
    return out


def time_calls(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--h', type=int, default=1080)
    ap.add_argument('--w', type=int, default=1920)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--oracle-batch', type=int, default=2)
    ap.add_argument('--only', choices=('default', 'given', 'hsv'), default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    n, h, w = a.batch, a.h, a.w
    px = n * h * w
    fl = ofl.Flow(smooth(n, h, w, 1, dev), 't')
    given = [float(4 + i % 5) for i in range(n)]
    res = {"op": "visualise", "batch": n, "h": h, "w": w, "iters": a.iters}
    # bytes: each histogram pass reads the flow (8 B/px); the colour pass reads it and writes 3 B/px
    model = {"default": 3 * 8 * px + 11 * px, "given": 11 * px, "hsv": 11 * px}
    calls = {"default": lambda: fl.visualise('bgr'), "given": lambda: fl.visualise('bgr', range_max=given),
             "hsv": lambda: fl.visualise('hsv')}
    for name in (a.only,) if a.only else ("default", "given", "hsv"):
        ms = time_calls(calls[name], a.iters if name != "hsv" else max(10, a.iters // 10), a.warmup)
        res[name] = {"ms": round(ms, 4), "bytes": model[name], "bytes_per_px": model[name] / px,
                     "share_of_8TBs": round(model[name] / (ms * 1e-3) / PEAK, 4)}
    if "hsv" in res:
        res["hsv"]["note"] = "returns a NumPy array: the time includes the device-to-host copy of the N-H-W-3 bytes"
    if a.oracle_batch > 0 and not a.only:
        import vis_oracle as vo
        v = fl.vecs[:a.oracle_batch].cpu().numpy()
        t0 = time.perf_counter()
        vo.visualise(v, 'bgr')
        res["numpy_oracle_ms"] = {"batch": a.oracle_batch, "ms": round((time.perf_counter() - t0) * 1e3, 1)}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
