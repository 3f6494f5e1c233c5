#!/usr/bin/env python3
"""Flow.matrix on the device: B = 64 1080p fp32 flows, every (dof, method) pair of the reference's test, timed by HIP events
over several calls after warm-up.

    python tools/bench_matrix.py [--batch 64] [--h 1080] [--w 1920] [--iters 10] [--warmup 2] [--oracle 1] [--only DOF:METHOD]

Prints one JSON line: ms per call of Flow.matrix (it ends in the read of N status words, so each call is synchronous), the
bytes the streaming passes move (computed from the shapes: 8 B/px per pass over an unmasked fp32 flow) and their rate beside
the box's device-copy rate measured in the same run, pixel-hypothesis evaluations per second for the robust methods, the time
with the outliers in the first and in the last image (K is fixed, there is no early exit), and the NumPy oracle's time for
one image.
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

PAIRS = [(4, 'ransac'), (4, 'lmeds'), (6, 'ransac'), (6, 'lmeds'), (8, 'lms'), (8, 'ransac'), (8, 'lmeds')]
K = {'ransac': 256, 'lmeds': 128, 'lms': 0}


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


def passes(dof, method):
    """streaming passes over the flow: hypothesis scoring (1 for RANSAC, 3 x K / 4 groups for LMedS) + the sums (1, or 2 for dof 8)"""
    score = {'lms': 0, 'ransac': 1, 'lmeds': 3 * (K['lmeds'] // 4)}[method]
    return score, (2 if dof == 8 else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--h', type=int, default=1080)
    ap.add_argument('--w', type=int, default=1920)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--oracle', type=int, default=1)
    ap.add_argument('--only', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    n, h, w = a.batch, a.h, a.w
    px = n * h * w
    from oflibpytorch_amd.utils import matrix_from_transforms
    mats = torch.stack([matrix_from_transforms([['translation', 2 + i % 7, 1 - i % 5], ['rotation', w / 5, h / 5, 10 - i % 9],
                                                ['scaling', w / 2, h / 2, 1.05 - 0.002 * i]]) for i in range(n)])
    vecs = ofl.Flow.from_matrix(mats, (h, w), 's', device=dev).vecs
    g = torch.Generator(device=dev).manual_seed(1)

    def with_outliers(images):
        v = vecs.clone()
        for i in images:
            bad = torch.rand(h, w, generator=g, device=dev) < 0.3
            v[i] = torch.where(bad, (torch.rand(2, h, w, generator=g, device=dev) - 0.5) * 200, v[i])
        return ofl.Flow(v, 's')

    fl = with_outliers(range(n))
    fl_first, fl_last = with_outliers([0]), with_outliers([n - 1])
    res = {"op": "matrix", "batch": n, "h": h, "w": w, "iters": a.iters}
    # the box's device-copy rate: a float32 tensor of the flow's size copied on the device (read + write)
    buf = torch.empty_like(vecs)
    ms_copy = time_calls(lambda: buf.copy_(vecs), 20, 3)
    res["device_copy_TBs"] = round(2 * 8 * px / (ms_copy * 1e-3) / 1e12, 3)
    for dof, method in PAIRS:
        name = "%d:%s" % (dof, method)
        if a.only and a.only != name:
            continue
        ms = time_calls(lambda: fl.matrix(dof, method), a.iters, a.warmup)
        score, sums = passes(dof, method)
        entry = {"ms": round(ms, 3), "sum_passes": sums, "score_passes": score, "bytes_sums": sums * 8 * px}
        if method == 'lms':
            entry["sums_TBs"] = round(sums * 8 * px / (ms * 1e-3) / 1e12, 3)
            entry["share_of_device_copy"] = round(entry["sums_TBs"] / res["device_copy_TBs"], 3)
        else:
            evals = px * K[method] * (1 if method == 'ransac' else 3)
            entry["pixel_hypothesis_evals"] = evals
            entry["evals_per_ns"] = round(evals / (ms * 1e6), 2)
            entry["ms_outliers_first_image"] = round(time_calls(lambda: fl_first.matrix(dof, method), max(2, a.iters // 2), 1), 3)
            entry["ms_outliers_last_image"] = round(time_calls(lambda: fl_last.matrix(dof, method), max(2, a.iters // 2), 1), 3)
        res[name] = entry
    if a.oracle > 0 and not a.only:
        import matrix_oracle as mo
        v1 = fl.vecs[:1].cpu().numpy()
        res["numpy_oracle_ms_one_image"] = {}
        for dof, method in PAIRS:
            t0 = time.perf_counter()
            mo.fit(v1, 's', None, dof, method)
            res["numpy_oracle_ms_one_image"]["%d:%s" % (dof, method)] = round((time.perf_counter() - t0) * 1e3, 1)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
