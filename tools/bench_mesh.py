#!/usr/bin/env python3
"""Flow.apply of an 's' flow through the triangle-mesh interpolator next to the splat in the same process: B = 16
1080p fp32, C = 3, on bench.py's sigma = 8 flow and on a smooth one (sigma = 2), timed by HIP events after warm-up.

    python tools/bench_mesh.py [--batch 16] [--h 1080] [--w 1920] [--iters 20] [--warmup 3] [--out profiles/mesh_bench.json]

Prints (and with --out writes) one JSON line: ms per call of Flow.apply in mesh mode and in splat mode for each flow, their ratio, the
list entries per quad of the mesh plan, and the kernels' own times as HIP events around the native call.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import torch  # noqa: E402

import oflibpytorch_amd as ofl  # noqa: E402
from oflibpytorch_amd import _native  # noqa: E402
from bench import smooth_flow  # noqa: E402
from bench_visualise import time_calls  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--h', type=int, default=1080)
    ap.add_argument('--w', type=int, default=1920)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    n, h, w = a.batch, a.h, a.w
    img = torch.rand(n, 3, h, w, device=dev)
    res = {"op": "Flow.apply 's', C=3, fp32", "batch": n, "h": h, "w": w, "iters": a.iters}
    for name, sigma in (("sigma8", 8.0), ("sigma2", 2.0)):
        fl = ofl.Flow(smooth_flow(n, h, w, sigma, 1000, dev), 's')
        fl.apply(img)                                            # (validation of the flow is cached from here on)
        entry = {}
        ofl.set_pure_pytorch()
        entry["splat_ms"] = round(time_calls(lambda: fl.apply(img), a.iters, a.warmup), 4)
        ofl.unset_pure_pytorch()
        ofl.set_mesh_interpolation()
        try:
            entry["mesh_ms"] = round(time_calls(lambda: fl.apply(img), a.iters, a.warmup), 4)
            entry["mesh_native_ms"] = round(time_calls(lambda: _native.mesh_apply(fl.vecs, img), a.iters, a.warmup), 4)
        finally:
            ofl.set_mesh_interpolation(False)
            ofl.set_pure_pytorch()
        entry["mesh_over_splat"] = round(entry["mesh_ms"] / entry["splat_ms"], 2)
        lib = _native.load_library()
        ws = torch.empty(int(lib.ofl_mesh_workspace_ints(n, h, w, 0)), dtype=torch.int32, device=dev)
        _native._check(lib.ofl_mesh_plan(_native._ptr(fl.vecs), fl.vecs.stride(0), 1.0, None, 0, 0, _native._ptr(ws), n, h, w,
                                         _native._stream(dev)), "ofl_mesh_plan")
        entry["list_entries_per_quad"] = round(int(ws[:2].view(torch.int64).item()) / (n * (h - 1) * (w - 1)), 4)
        res[name] = entry
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
