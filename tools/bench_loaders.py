#!/usr/bin/env python3
"""Flow.from_kitti on a batch of KITTI-sized frames: the device route next to the reference's host route in the same
process, and the decode kernel on its own next to the box's device-copy rate.

    python tools/bench_loaders.py [--batch 16] [--h 375] [--w 1242] [--iters 10] [--warmup 2] [--sets 12] [--out profiles/loaders_bench.json]

The frames are synthetic (a smooth flow quantised the KITTI way, every third pixel invalid), written to a temporary directory as
16-bit RGB PNGs by the small encoder below (Sub filter, zlib level 6).  Prints (and with --out writes) one JSON line:
  new_ms            Flow.from_kitti(list of paths, device='cuda'): read, inflate, unfilter (thread pool), one upload, one kernel
  host_route_ms     the same files decoded by this package's host decoder, then the NumPy conversion as the reference writes it
                    (utils.py:826-829) and Flow(vecs, 's', mask, device='cuda') per frame, batched with batch_flows
  host_decode_ms    read + inflate + unfilter alone (both routes pay it)
  binding_call_us   _native.decode_kitti by HIP events: three allocations, the flag memset and the launch, on one cache-resident input
  kernel_us, kernel_gbs     ofl_decode_kitti through the C ABI on preallocated outputs (flag memset included), by HIP events, rotating over
                    --sets separate inputs and outputs (12 x 112 MB, several times the last-level cache); bytes: 6 in + 9 out per pixel
  copy_us, copy_gbs  a device-to-device copy of as many bytes in all (read + write), rotating over as many buffer pairs, same events
"""
import argparse
import json
import os
import struct
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import oflibpytorch_amd as ofl  # noqa: E402
from oflibpytorch_amd import _loaders, _native  # noqa: E402


def write_png16(path, samples):
    """[H, W, 3] uint16 -> a 16-bit RGB PNG, every row Sub-filtered (vectorised: the difference to the pixel on the left)."""
    h, w, _ = samples.shape
    rows = samples.astype('>u2').view(np.uint8).reshape(h, w * 6).astype(np.int16)
    rows[:, 6:] -= rows[:, :-6].copy()
    body = np.concatenate([np.ones((h, 1), np.uint8), (rows & 0xff).astype(np.uint8)], axis=1).tobytes()
    chunk = lambda t, b: struct.pack('>I', len(b)) + t + b + struct.pack('>I', zlib.crc32(t + b) & 0xffffffff)
    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 16, 2, 0, 0, 0)) + chunk(b'IDAT', zlib.compress(body, 6))
                + chunk(b'IEND', b''))


def frame(h, w, seed):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    u = 20 * np.sin(xx / 97.0 + seed) + rng.randn(h, w) * 0.25
    v = 8 * np.cos(yy / 61.0 - seed) + rng.randn(h, w) * 0.25
    s = np.zeros((h, w, 3), dtype=np.uint16)
    s[..., 0] = np.clip(np.rint(u * 64 + 2 ** 15), 0, 65535)
    s[..., 1] = np.clip(np.rint(v * 64 + 2 ** 15), 0, 65535)
    s[..., 2] = (rng.rand(h, w) < 2 / 3)
    s[s[..., 2] == 0, :2] = 0                        # KITTI stores zeros where there is no ground truth
    return s


def wall(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


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


def host_route(paths, dev):
    flows = []
    for p in paths:
        img = _loaders.decode_png(open(p, 'rb').read())
        inp = img.raw.reshape(img.height, img.width, 3, 2)
        inp = (inp[..., 0].astype(np.uint16) << 8 | inp[..., 1]).astype('float64')        # what cv2.imread hands over, as R G B
        inp[..., :2] = (inp[..., :2] - 2 ** 15) / 64
        inp[inp[..., 2] > 0, 2] = 1
        data = torch.tensor(np.moveaxis(inp, -1, 0)).float()
        flows.append(ofl.Flow(data[:2], 's', data[2], device=dev))
    return ofl.batch_flows(flows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--h', type=int, default=375)
    ap.add_argument('--w', type=int, default=1242)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sets', type=int, default=12)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    n, h, w = a.batch, a.h, a.w
    with tempfile.TemporaryDirectory(prefix="ofl_loaders_") as tmp:
        paths = [os.path.join(tmp, "%06d_10.png" % i) for i in range(n)]
        for i, p in enumerate(paths):
            write_png16(p, frame(h, w, i))
        new = ofl.Flow.from_kitti(paths, device=dev)
        old = host_route(paths, dev)
        same = bool(torch.equal(new.vecs.view(torch.int32), old.vecs.view(torch.int32)) and torch.equal(new.mask, old.mask))
        res = {"op": "Flow.from_kitti", "batch": n, "h": h, "w": w, "iters": a.iters, "file_bytes": sum(os.path.getsize(p) for p in paths),
               "routes_agree_bit_for_bit": same}
        res["new_ms"] = round(wall(lambda: ofl.Flow.from_kitti(paths, device=dev), a.iters, a.warmup), 3)
        res["host_route_ms"] = round(wall(lambda: host_route(paths, dev), a.iters, a.warmup), 3)
        res["host_decode_ms"] = round(wall(lambda: _loaders._map(lambda p: _loaders.decode_png(open(p, 'rb').read()), paths), a.iters, a.warmup), 3)
        res["host_decode_one_thread_ms"] = round(wall(lambda: [_loaders.decode_png(open(p, 'rb').read()) for p in paths], a.iters, a.warmup), 3)
        raw = torch.stack([torch.from_numpy(_loaders.decode_png(open(p, 'rb').read()).raw.reshape(-1)) for p in paths]).to(dev)
    # the binding as a caller meets it: three allocations, the flag memset, the launch -- on ONE input that stays in the last-level cache
    res["binding_call_us"] = round(events(lambda: _native.decode_kitti(raw, h, w, True), 50, 5), 2)
    # the kernel (with its flag memset) through the C ABI on preallocated outputs, rotating over `sets` separate inputs and outputs whose
    # total is several times the 256 MB last-level cache, so that every call reads and writes memory; the copy rotates the same way
    nbytes, sets = n * h * w * 15, a.sets
    lib, st = _native.load_library(), _native._stream(dev)
    raws = [raw.clone() for _ in range(sets)]
    outs = [(torch.empty((n, 2, h, w), dtype=torch.float32, device=dev), torch.empty((n, h, w), dtype=torch.bool, device=dev),
             torch.empty(n, dtype=torch.int32, device=dev)) for _ in range(sets)]
    turn = [0]

    def kernel_call():
        i = turn[0] = (turn[0] + 1) % sets
        v, m, f = outs[i]
        _native._check(lib.ofl_decode_kitti(_native._ptr(raws[i]), raws[i].stride(0), _native._ptr(v), _native._ptr(m), _native._ptr(f), n, h, w, st),
                       "ofl_decode_kitti")

    res["kernel_us"] = round(events(kernel_call, 10 * sets, 2 * sets), 2)
    res["kernel_gbs"] = round(nbytes / res["kernel_us"] / 1e3, 1)
    pairs = [(torch.empty(nbytes // 2, dtype=torch.uint8, device=dev), torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)) for _ in range(sets)]

    def copy_call():
        i = turn[0] = (turn[0] + 1) % sets
        pairs[i][1].copy_(pairs[i][0])

    res["copy_us"] = round(events(copy_call, 10 * sets, 2 * sets), 2)
    res["copy_gbs"] = round(nbytes // 2 * 2 / res["copy_us"] / 1e3, 1)
    res["rotating_sets"], res["bytes_per_call"], res["kernel"] = sets, nbytes, "decode_kitti_kernel"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + "\n")


if __name__ == '__main__':
    main()
