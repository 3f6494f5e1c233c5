#!/usr/bin/env python3
"""Flow.apply 't' of a channels_last feature tensor on the N-H-W-C kernel next to what the planar route costs for the
same input, in ONE process: B = 8 1080p on bench.py's sigma = 8 flow, fp32 and bf16, C = 64 and C = 4, 8, 16, 32, timed by HIP events
after warm-up.  Three things are timed per (dtype, C), alternating over `--rounds` rounds so that the run-to-run spread is in the file:

    (a) native       Flow.apply(target)                                      -- the channels_last route
    (b) planar       Flow.apply(target.contiguous())                         -- what the planar route does for that input (result N-C-H-W)
    (c) planar_back  (b) + .contiguous(memory_format=torch.channels_last)    -- what a channels_last model pays on the planar route

    python tools/bench_nhwc.py [--batch 8] [--h 1080] [--w 1920] [--channels 64,4,8,16,32] [--dtypes float32,bfloat16]
                               [--iters 20] [--warmup 3] [--rounds 5] [--out profiles/nhwc_bench.json]

With --backward the BACKWARD of that call is timed instead (DESIGN.md 3.14 "Autograd"): the forward runs once outside the timing, then
`torch.autograd.grad(out, inputs, g, retain_graph=True)` with a channels_last upstream gradient `g` (native: ofl_warp_bwd_grad_nhwc and the
library's layout copies around the gather splat) alternates with the same call on `g.contiguous()`, which takes the planar backward with
ATen's strided copies -- what the route cost before for the same input.  Three variants per (dtype, C): flow and target both requiring a
gradient, only the flow, only the target.  The two layout copies are timed on their own next to a same-layout device copy of the same
tensor (`copy_`), as bytes moved (read + write) per second.

    python tools/bench_nhwc.py --backward [--channels 4,8,16,32,64] [--out profiles/nhwc_backward_bench.json]

Prints (and with --out writes) one JSON line.  Per entry: median / min / max ms per call of each of the three, the share of the
8 TB/s roofline of (a) on the kernel's own bytes (source read once + result written once + the fp32 flow), the ratios (b) / (a) and
(c) / (a) of the medians, and whether (a) and (b) gave the same bits.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import torch  # noqa: E402

import oflibpytorch_amd as ofl  # noqa: E402
from oflibpytorch_amd import _native  # noqa: E402
from bench import smooth_flow  # noqa: E402
from bench_visualise import time_calls  # noqa: E402

PEAK_BYTES_PER_S = 8e12
CL = torch.channels_last


def _stat(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def backward_leg(a, dev):
    n, h, w = a.batch, a.h, a.w
    vecs = smooth_flow(n, h, w, 8.0, 1000, dev)
    res = {"op": "backward of Flow.apply 't' of a channels_last tensor, channels_last upstream gradient", "batch": n, "h": h, "w": w,
           "sigma": 8.0, "iters": a.iters, "rounds": a.rounds, "entries": []}
    variants = {"both": (True, True), "flow_only": (True, False), "target_only": (False, True)}
    for dtype in [getattr(torch, d) for d in a.dtypes.split(',')]:
        for c in [int(v) for v in a.channels.split(',')]:
            t = torch.rand(n, c, h, w, device=dev).to(dtype).contiguous(memory_format=CL)
            g = torch.randn(n, c, h, w, device=dev).to(dtype).contiguous(memory_format=CL)
            elem = t.element_size()
            entry = {"dtype": str(dtype).replace("torch.", ""), "c": c, "map_bytes": n * c * h * w * elem}
            for name, (wf, wt) in variants.items():
                v1 = vecs.clone().requires_grad_(wf)
                t1 = t.clone(memory_format=torch.preserve_format).requires_grad_(wt)
                out = ofl.Flow(v1, 't').apply(t1)
                inputs = [x for x, on in ((v1, wf), (t1, wt)) if on]
                routes = {"native": lambda: torch.autograd.grad(out, inputs, g, retain_graph=True),
                          "planar": lambda: torch.autograd.grad(out, inputs, g.contiguous(), retain_graph=True)}
                got = routes["native"]()
                kernel = _native.last_kernel_name()
                if "warp_grad_flow_nhwc_kernel" not in kernel and "nhwc_transpose_kernel" not in kernel:
                    raise RuntimeError("the channels_last backward did not run for C = %d %s %s (%s)" % (c, dtype, name, kernel))
                ref = routes["planar"]()
                same = all(x.dtype == y.dtype and bool(torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)))
                           for x, y in zip(got, ref))
                del got, ref
                ms = {k: [] for k in routes}
                for _ in range(a.rounds):                              # alternate the two: one box, shared with other work
                    for k, fn in routes.items():
                        ms[k].append(time_calls(fn, a.iters, a.warmup))
                entry[name] = {"kernel": kernel, "same_bits_as_planar": same, "native_ms": _stat(ms["native"]), "planar_ms": _stat(ms["planar"]),
                               "planar_over_native": round(statistics.median(ms["planar"]) / statistics.median(ms["native"]), 3),
                               # the route is taken where even the slowest native round beats the fastest planar round
                               "native_max_over_planar_min": round(max(ms["native"]) / min(ms["planar"]), 3)}
                del out, v1, t1, inputs
            gp = g.contiguous()
            dst = torch.empty_like(gp)
            copies = {"nhwc_to_planes": lambda: _native.nhwc_to_planes(g), "planes_to_nhwc": lambda: _native.planes_to_nhwc(gp),
                      "device_copy": lambda: dst.copy_(gp), "aten_to_planes": lambda: g.contiguous(),
                      "aten_to_nhwc": lambda: gp.contiguous(memory_format=CL)}
            cms = {k: [] for k in copies}
            for _ in range(a.rounds):
                for k, fn in copies.items():
                    cms[k].append(time_calls(fn, a.iters, a.warmup))
            entry["copies"] = {k: dict(_stat(v), bytes_per_s=round(2 * entry["map_bytes"] / (statistics.median(v) * 1e-3), -6)) for k, v in cms.items()}
            res["entries"].append(entry)
            print(json.dumps(entry), file=sys.stderr, flush=True)
            del t, g, gp, dst
            torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--backward', action='store_true')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--h', type=int, default=1080)
    ap.add_argument('--w', type=int, default=1920)
    ap.add_argument('--channels', default='64,4,8,16,32')
    ap.add_argument('--dtypes', default='float32,bfloat16')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    if a.backward:
        res = backward_leg(a, dev)
    else:
        res = forward_leg(a, dev)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + "\n")


def forward_leg(a, dev):
    n, h, w = a.batch, a.h, a.w
    fl = ofl.Flow(smooth_flow(n, h, w, 8.0, 1000, dev), 't')
    res = {"op": "Flow.apply 't' of a channels_last tensor", "batch": n, "h": h, "w": w, "sigma": 8.0, "iters": a.iters,
           "rounds": a.rounds, "roofline_bytes_per_s": PEAK_BYTES_PER_S, "entries": []}
    for dtype in [getattr(torch, d) for d in a.dtypes.split(',')]:
        for c in [int(v) for v in a.channels.split(',')]:
            t = torch.rand(n, c, h, w, device=dev).to(dtype).contiguous(memory_format=CL)
            routes = {"native": lambda: fl.apply(t),
                      "planar": lambda: fl.apply(t.contiguous()),
                      "planar_back": lambda: fl.apply(t.contiguous()).contiguous(memory_format=CL)}
            got = routes["native"]()
            kernel = _native.last_kernel_name()
            if "warp_bwd_nhwc_kernel" not in kernel:
                raise RuntimeError("the channels_last route did not run for C = %d %s (%s)" % (c, dtype, kernel))
            ref = routes["planar"]()
            bits = torch.int32 if dtype == torch.float32 else torch.int16
            same = bool(torch.equal(got.contiguous().view(bits), ref.view(bits))) and got.is_contiguous(memory_format=CL)
            planar_kernel = _native.last_kernel_name()
            del got, ref
            ms = {k: [] for k in routes}
            for _ in range(a.rounds):                                  # alternate the three: one box, shared with other work
                for k, fn in routes.items():
                    ms[k].append(time_calls(fn, a.iters, a.warmup))
            elem = torch.zeros((), dtype=dtype).element_size()
            own_bytes = n * h * w * (2 * c * elem + 8)
            entry = {"dtype": str(dtype).replace("torch.", ""), "c": c, "kernel": kernel, "planar_kernel": planar_kernel,
                     "same_bits_as_planar": same, "own_bytes": own_bytes}
            for k, v in ms.items():
                entry[k + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
            med = {k: statistics.median(v) for k, v in ms.items()}
            entry["native_roofline_share"] = round(own_bytes / PEAK_BYTES_PER_S / (med["native"] * 1e-3), 4)
            entry["planar_over_native"] = round(med["planar"] / med["native"], 3)
            entry["planar_back_over_native"] = round(med["planar_back"] / med["native"], 3)
            # (a) is "not slower than (b)" when even its slowest round is within the fastest round of (b)
            entry["native_max_over_planar_min"] = round(max(ms["native"]) / min(ms["planar"]), 3)
            res["entries"].append(entry)
            print(json.dumps(entry), file=sys.stderr, flush=True)
            del t
            torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    main()
