#!/usr/bin/env python3
"""Backward warp (apply_flow 't') of a feature tensor stored in fp32, bf16 and fp16: the 16-bit calls run the 16-bit instantiations of
the staged kernels (ofl_warp_bwd_x16: 2 C + 8 B/px read, 2 C B/px written) where the library has them, and the copy route
(`.float()`, the fp32 kernel, `.to(dtype)`) where it does not -- the same script times both, e.g. on two check-outs.
Per configuration: the median of 5 blocks of 100 calls (one event pair round each block, as bench.py --full), the five block times,
the kernel the library reports, the fraction of 8 TB/s on the call's own algorithmic bytes; the box's device-copy rate on top.

    python tools/bench_half_warp.py [--label result] [--out profiles/half_warp_bench.json] [--iters 100] [--sigma 8] [--backward]
    (--out appends this run under --label to the runs already in the file)

--backward times a TRAINING step instead: forward + backward of apply_flow 't' at B = 8, C = 64, with the target and the flow both
requiring gradients, in fp32 / bf16 / fp16 -- the same blocks, and next to the time the peak of torch.cuda.max_memory_allocated over
one step above the level before it.  Where the library has the native 16-bit backward (ofl_warp_bwd_grad_x16, ofl_splat_sum_x16) the
16-bit steps run it; on a check-out without it they run the copy route.  Its run is stored under "<label>-backward"."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench
import oflibpytorch_amd as ofl
from oflibpytorch_amd import _native

ap = argparse.ArgumentParser()
ap.add_argument("--label", default="result")
ap.add_argument("--out", default=None)
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--sigma", type=float, default=8.0)
ap.add_argument("--configs", type=int, nargs="+", default=[8, 64, 64, 3], help="pairs B C")
ap.add_argument("--backward", action="store_true", help="time forward + backward (B = 8, C = 64) and report the peak memory of a step")
a = ap.parse_args()
if a.backward:
    a.label, a.configs = a.label + "-backward", [8, 64]
dev = torch.device('cuda', 0)
h, w = 1080, 1920
_native.load_library()
copy_gbs, _ = bench.stream_probes(dev)


def blocks_ms(fn, iters, blocks=5, warm=10):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / iters)
    return sorted(t)


run = {"label": a.label, "device": torch.cuda.get_device_name(dev), "device_copy_GBps": round(copy_gbs, 1), "iters": a.iters,
       "sigma": a.sigma, "frame": [h, w], "cases": []}
for n, C in zip(a.configs[0::2], a.configs[1::2]):
    f = bench.smooth_flow(n, h, w, a.sigma, 1003, dev)
    feat32 = torch.rand(n, C, h, w, device=dev) * 2 - 1
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        if a.backward:
            feat = feat32.to(dt).requires_grad_(True)
            fl = f.clone().requires_grad_(True)
            g = (torch.rand(n, C, h, w, device=dev) - 0.5).to(dt)

            def step():
                feat.grad = fl.grad = None
                ofl.apply_flow(fl, feat, 't').backward(g)
            step()
            kernel = _native.last_kernel_name()                        # (the last launch of the backward pass)
            assert feat.grad.dtype == dt and fl.grad.dtype == torch.float32
            torch.cuda.synchronize()
            feat.grad = fl.grad = None
            torch.cuda.reset_peak_memory_stats(dev)
            level = torch.cuda.memory_allocated(dev)
            step()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated(dev) - level
            t = blocks_ms(step, a.iters)
            case = {"B": n, "C": C, "dtype": str(dt).replace("torch.", ""), "step": "forward+backward", "ms_median": round(t[2], 4),
                    "ms_blocks": [round(x, 4) for x in t], "peak_bytes_over_step": int(peak),
                    "peak_bytes_per_element": round(peak / feat.numel(), 2), "kernel": kernel}
            run["cases"].append(case)
            print("B=%2d C=%2d %-8s fwd+bwd %.3f ms (blocks %.3f .. %.3f)  peak %.2f GB = %.1f B/element   %s"
                  % (n, C, case["dtype"], t[2], t[0], t[-1], peak / 1e9, peak / feat.numel(), kernel), flush=True)
            del feat, fl, g
            torch.cuda.empty_cache()
            continue
        feat = feat32.to(dt)
        out = ofl.apply_flow(f, feat, 't')
        kernel = _native.last_kernel_name()
        assert out.dtype == dt
        t = blocks_ms(lambda: ofl.apply_flow(f, feat, 't'), a.iters)
        eb = 2 if dt != torch.float32 else 4
        bpp = 8 + 2 * eb * C                                        # flow read once, every plane read once and written once
        case = {"B": n, "C": C, "dtype": str(dt).replace("torch.", ""), "ms_median": round(t[2], 4), "ms_blocks": [round(x, 4) for x in t],
                "bytes_per_px": bpp, "frac_of_8TBps": round(bpp * n * h * w / (t[2] * 1e-3) / 8e12, 3), "kernel": kernel}
        run["cases"].append(case)
        print("B=%2d C=%2d %-8s %.3f ms (blocks %.3f .. %.3f)  %.3f of 8 TB/s on %d B/px   %s"
              % (n, C, case["dtype"], t[2], t[0], t[-1], case["frac_of_8TBps"], bpp, kernel), flush=True)
        del feat, out
    del feat32, f
    torch.cuda.empty_cache()
print(json.dumps(run))
if a.out:
    doc = {"runs": []}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            doc = json.load(fh)
    doc["runs"] = [r for r in doc["runs"] if r["label"] != a.label] + [run]
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
