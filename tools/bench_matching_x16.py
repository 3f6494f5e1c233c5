#!/usr/bin/env python3
"""Flow.from_matching on fp16 / bf16 features next to what a user had before it -- the same features converted to
float32 and matched by the float32 route, conversions included -- and next to the eager composition (matmul into the (H W)^2 volume,
softmax over it, matmul with the coordinate grid) in the same 16-bit dtype and in float32, all in one process.

    python tools/bench_matching_x16.py [--case full|crop|both] [--dtype bf16|fp16|both] [--batch 8] [--channels 128] [--iters 3]
                                       [--warmup 1] [--blocks 5] [--out profiles/matching_x16_bench.json]

Cases: `full` 135 x 240 and `crop` 48 x 96, B = 8 and C = 128 by default; the features are N(0, 1) rounded to the dtype, the upstream
gradient uniform in [-1, 1).  Every time is the median of `blocks` blocks of `iters` calls each, after `warmup` calls, by HIP events;
`*_spread_us` is the largest minus the smallest block.  Peak memory is torch.cuda.max_memory_allocated beyond what was allocated before
the call (the inputs).  The eager compositions run on the first `eager_images` images (as many as leave three float32 volumes an image
under half the device's free memory); ratios to them compare per image.  Prints one JSON line per case and dtype and with --out writes
{case: {dtype: result}} (an existing file keeps its other entries):
  fwd_us, fwd_bwd_us, *_peak_bytes           Flow.from_matching(feat16, other16, 's', return_prob=True); ... and .vecs.backward(g)
  f32_fwd_us, f32_fwd_bwd_us, ...            Flow.from_matching(feat16.float(), other16.float(), ...): the float32 route, conversions included
  x16_faster_fwd                             f32_fwd_us - fwd_us > f32_fwd_spread_us + fwd_spread_us: the ordering DESIGN.md 3.32 requires
  eager16_*, eager32_*                       the eager composition in the dtype / in float32 on `eager_images` images
  fwd_tflops, fwd_frac_mfma_peak             2 C (H W)^2 flops an image over fwd_us; over 2516.8 TFLOPS, the dense bf16 / fp16 MFMA peak
  max_abs_diff_f64, f32_max_abs_diff_f64     the largest difference of the flow to the float64 evaluation of the same 16-bit values, on
                                             `sample` pixels of image 0 (this route; the float32 route)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import oflibpytorch_amd as ofl  # noqa: E402
from tools.bench_matching import CASES, eager_expression, events, peak  # noqa: E402

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
MFMA_PEAK_TFLOPS = 16 * 157.3                # dense bf16 / fp16 MFMA: 16 times the float32 vector peak


def float64_sample(feat, other, idx):
    """The flow of an 's' flow at the pixels `idx` of image 0, in float64 on the exact values of the 16-bit features: [2, len(idx)]"""
    _, c, h, w = feat.shape
    f = feat[0].double().view(c, h * w)[:, idx]
    o = other[0].double().view(c, h * w)
    p = torch.softmax(f.t() @ o / (c ** 0.5), dim=1)
    q = torch.arange(h * w, device=feat.device)
    grid = torch.stack([q % w, q // w], 1).double()
    return (p @ grid - grid[idx]).t()


def measure(name, kind, n, c, a, dev):
    h, w = CASES[name]
    dtype = DTYPES[kind]
    gen = torch.Generator(device=dev).manual_seed(11)
    feat = torch.randn((n, c, h, w), device=dev, generator=gen).to(dtype)
    other = torch.randn((n, c, h, w), device=dev, generator=gen).to(dtype)
    g = torch.rand((n, 2, h, w), device=dev, generator=gen) * 2 - 1
    timed = lambda fn: events(fn, a.iters, a.warmup, a.blocks)
    volume = 4 * (h * w) ** 2
    res = {"case": name, "features": kind, "batch": n, "channels": c, "h": h, "w": w, "volume_bytes_per_image": volume}
    f_g, o_g = feat.clone().requires_grad_(), other.clone().requires_grad_()

    def route(convert, key):
        cast = (lambda t: t.float()) if convert else (lambda t: t)
        fwd = lambda: ofl.Flow.from_matching(cast(feat), cast(other), 's', return_prob=True)
        (flow, _), res[key + "fwd_peak_bytes"] = peak(fwd, dev)
        res[key + "fwd_us"], res[key + "fwd_spread_us"] = timed(fwd)

        def fwd_bwd():
            f_g.grad, o_g.grad = None, None
            ofl.Flow.from_matching(cast(f_g), cast(o_g), 's').vecs.backward(g)

        _, res[key + "fwd_bwd_peak_bytes"] = peak(fwd_bwd, dev)
        res[key + "fwd_bwd_us"], res[key + "fwd_bwd_spread_us"] = timed(fwd_bwd)
        assert f_g.grad.dtype == dtype and o_g.grad.dtype == dtype
        f_g.grad, o_g.grad = None, None
        return flow.vecs.detach()

    flow16 = route(False, "")
    flow32 = route(True, "f32_")
    res["fwd_tflops"] = round(2.0 * c * (h * w) ** 2 * n / res["fwd_us"] / 1e6, 2)
    res["fwd_frac_mfma_peak"] = round(res["fwd_tflops"] / MFMA_PEAK_TFLOPS, 4)
    res["x16_faster_fwd"] = bool(res["f32_fwd_us"] - res["fwd_us"] > res["f32_fwd_spread_us"] + res["fwd_spread_us"])
    res["x16_faster_fwd_bwd"] = bool(res["f32_fwd_bwd_us"] - res["fwd_bwd_us"] > res["f32_fwd_bwd_spread_us"] + res["fwd_bwd_spread_us"])
    res["time_ratio_fwd_to_f32"] = round(res["fwd_us"] / res["f32_fwd_us"], 4)
    res["time_ratio_fwd_bwd_to_f32"] = round(res["fwd_bwd_us"] / res["f32_fwd_bwd_us"], 4)
    # the float64 evaluation on a subsample of image 0
    idx = torch.randperm(h * w, device=dev, generator=gen)[:a.sample]
    want = float64_sample(feat, other, idx)
    res["sample"] = int(idx.numel())
    res["max_abs_diff_f64"] = float((flow16[0].view(2, -1)[:, idx].double() - want).abs().max())
    res["f32_max_abs_diff_f64"] = float((flow32[0].view(2, -1)[:, idx].double() - want).abs().max())
    del want, flow16, flow32
    # the eager compositions, on as many images as fit
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info(dev)[0]
    k = max(1, min(n, int(free // 2 // (3 * volume))))
    res["device_free_bytes"], res["eager_images"] = int(free), k
    for key, cast in (("eager16_", lambda t: t), ("eager32_", lambda t: t.float())):
        fe, oe = cast(feat[:k]).detach().clone().requires_grad_(), cast(other[:k]).detach().clone().requires_grad_()
        ge = g[:k].to(fe.dtype).contiguous()
        with torch.no_grad():
            _, res[key + "fwd_peak_bytes"] = peak(lambda: eager_expression(fe, oe), dev)
            res[key + "fwd_us"], res[key + "fwd_spread_us"] = timed(lambda: eager_expression(fe, oe))

        def eager_fwd_bwd():
            fe.grad, oe.grad = None, None
            eager_expression(fe, oe)[0].backward(ge)

        _, res[key + "fwd_bwd_peak_bytes"] = peak(eager_fwd_bwd, dev)
        res[key + "fwd_bwd_us"], res[key + "fwd_bwd_spread_us"] = timed(eager_fwd_bwd)
        for what in ("fwd", "fwd_bwd"):
            res["time_ratio_%s_to_%s" % (what, key[:-1])] = round((res[what + "_us"] / n) / (res[key + what + "_us"] / k), 3)
            res["mem_ratio_%s_to_%s" % (what, key[:-1])] = round((res[what + "_peak_bytes"] / n) / (res[key + what + "_peak_bytes"] / k), 6)
        del fe, oe, ge
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='both', choices=('full', 'crop', 'both'))
    ap.add_argument('--dtype', default='both', choices=('bf16', 'fp16', 'both'))
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--channels', type=int, default=128)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--sample', type=int, default=512)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    done = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            done = json.load(f)
    for name in (('crop', 'full') if a.case == 'both' else (a.case,)):
        for kind in (('bf16', 'fp16') if a.dtype == 'both' else (a.dtype,)):
            res = {"op": "Flow.from_matching", "ref": "s", "iters": a.iters, "warmup": a.warmup, "blocks": a.blocks}
            res.update(measure(name, kind, a.batch, a.channels, a, dev))
            print(json.dumps(res), flush=True)
            done.setdefault(name, {})[kind] = res
            if a.out:
                with open(a.out, 'w') as f:
                    f.write(json.dumps(done, indent=1, sort_keys=True) + "\n")


if __name__ == '__main__':
    main()
