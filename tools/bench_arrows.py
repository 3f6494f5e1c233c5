#!/usr/bin/env python3
"""Flow.visualise_arrows on the device: B = 64 1080p fp32 flows, grid_dist 20, thickness 1, default scaling, ref 't', timed by
HIP events over many calls after warm-up.

    python tools/bench_arrows.py [--batch 64] [--h 1080] [--w 1920] [--grid-dist 20] [--iters 50] [--warmup 5] [--oracle 1]
                                 [--only white|img|yardstick]

Prints one JSON line: ms per call of (a) visualise_arrows with img=None, (b) with a device uint8 img, (c) the yardstick
Flow.visualise('bgr', range_max=given) on the same flows (it also writes 3 B/px of uint8; it reads 8 B/px of flow where (b) reads
3 B/px of background), the ratio (b) / (c), the bytes each moves (computed from the shapes), the box's device-copy rate measured
in the same run, and the NumPy oracle's time for one image of the same input (the host baseline).
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
from bench_visualise import smooth, time_calls  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--h', type=int, default=1080)
    ap.add_argument('--w', type=int, default=1920)
    ap.add_argument('--grid-dist', type=int, default=20)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--oracle', type=int, default=1)
    ap.add_argument('--only', choices=('white', 'img', 'yardstick'), default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    n, h, w, g = a.batch, a.h, a.w, a.grid_dist
    px = n * h * w
    vecs = smooth(n, h, w, 1, dev)
    fl = ofl.Flow(vecs, 't')
    img = torch.randint(0, 256, (n, 3, h, w), dtype=torch.uint8, device=dev)
    given = [float(4 + i % 5) for i in range(n)]
    points = n * len(range(g // 2, h - 1, g)) * len(range(g // 2, w - 1, g))
    res = {"op": "visualise_arrows", "batch": n, "h": h, "w": w, "grid_dist": g, "thickness": 1, "ref": "t", "iters": a.iters,
           "arrows": points}
    # the box's device-copy rate: a float32 tensor of the flow's size copied on the device (read + write)
    buf = torch.empty_like(vecs)
    ms_copy = time_calls(lambda: buf.copy_(vecs), 20, 3)
    res["device_copy_TBs"] = round(2 * 8 * px / (ms_copy * 1e-3) / 1e12, 3)
    del buf
    # bytes: (a) writes 3 B/px; (b) reads 3 and writes 3 B/px; both read the flow at the grid points only and write / read one
    # 80-byte record per arrow; (c) reads 8 B/px of flow and writes 3 B/px
    model = {"white": 3 * px + 2 * 80 * points, "img": 6 * px + 2 * 80 * points, "yardstick": 11 * px}
    calls = {"white": lambda: fl.visualise_arrows(g), "img": lambda: fl.visualise_arrows(g, img),
             "yardstick": lambda: fl.visualise('bgr', range_max=given)}
    for name in (a.only,) if a.only else ("white", "img", "yardstick"):
        ms = time_calls(calls[name], a.iters, a.warmup)
        res[name] = {"ms": round(ms, 4), "bytes": model[name], "bytes_per_px": round(model[name] / px, 3),
                     "TBs": round(model[name] / (ms * 1e-3) / 1e12, 3)}
    if "img" in res and "yardstick" in res:
        res["img_over_yardstick"] = round(res["img"]["ms"] / res["yardstick"]["ms"], 3)
    if a.oracle > 0 and not a.only:
        import arrows_oracle as ao
        v1 = vecs[:a.oracle].cpu().numpy()
        bg = np.ascontiguousarray(np.moveaxis(img[:a.oracle].cpu().numpy(), 1, -1))
        t0 = time.perf_counter()
        ao.visualise_arrows(v1, 't', None, g, bg)
        res["numpy_oracle_ms"] = {"batch": a.oracle, "ms": round((time.perf_counter() - t0) * 1e3, 1)}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
