#!/usr/bin/env python3
"""Generate tests/golden/vis.npz by running the REFERENCE's Flow.visualise / visualise_flow (oflibpytorch v2.1.1, PyTorch CPU)
on small deterministic flows.

Runs only where the reference's sources exist (like gen_golden.py).  OpenCV is not installed there, so a stand-in `cv2` module
provides the three calls visualise makes: cartToPolar (OpenCV 4.x's FMA path, restated in tests/vis_oracle.py) and
findContours / drawContours (the 0-framed border pixels of the mask).  Everything else -- percentile, promotions, HSV -> RGB,
return types, the 'hsv' quirk -- is the reference's own NumPy code, which these fixtures pin.

    python tests/golden/gen_visualise.py [path to the reference's src/]

Each case k stores  c{k}_out (uint8, as returned: N-H-W-3 array, or N-3-H-W tensor) and c{k}_meta = json {mode, show_mask,
show_mask_borders, range_max, return_tensor, api, tensor, error, returned, flow, mask}, where flow / mask name the input arrays
(in_<hash>; mask None: the flow has none).
"""
import hashlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import vis_oracle as vo  # noqa: E402


def _cv2_stand_in():
    m = types.ModuleType('cv2')
    m.RETR_TREE, m.CHAIN_APPROX_SIMPLE = 3, 2

    def cartToPolar(x, y, angleInDegrees=False):
        assert angleInDegrees
        return vo.cart_to_polar(np.ascontiguousarray(x), np.ascontiguousarray(y))

    def findContours(img, mode, method):
        pts = np.argwhere(vo.mask_borders(img != 0))           # (row, col)
        return [pts[:, ::-1].reshape(-1, 1, 2).astype(np.int32)], None

    def drawContours(img, contours, idx, color, thickness):
        assert idx == -1 and thickness == 1
        for c in contours:
            c = c.reshape(-1, 2)
            img[c[:, 1], c[:, 0]] = color
        return img

    m.cartToPolar, m.findContours, m.drawContours = cartToPolar, findContours, drawContours
    return m


def main():
    src = sys.argv[1] if len(sys.argv) > 1 else '/root/reference/src'
    sys.modules['cv2'] = _cv2_stand_in()
    sys.path.insert(0, src)
    import oflibpytorch as of

    rs = np.random.RandomState(11)
    store, k = {}, 0

    def put(a):                      # inputs shared between cases are stored once
        key = 'in_' + hashlib.sha1(a.tobytes() + str((a.dtype, a.shape)).encode()).hexdigest()[:16]
        store[key] = a
        return key

    def smooth(n, h, w, scale):
        lo = rs.randn(n, 2, 4, 5).astype(np.float32) * scale
        t = torch.nn.functional.interpolate(torch.from_numpy(lo), size=(h, w), mode='bicubic', align_corners=True)
        return t.numpy().astype(np.float32)

    def rec(flow, mask, api='flow', tensor=True, **kw):
        nonlocal k
        meta = dict(kw, api=api, tensor=tensor)
        fin = torch.from_numpy(flow) if tensor else flow
        try:
            if api == 'flow':
                out = of.Flow(fin, 't', None if mask is None else torch.from_numpy(mask)).visualise(**kw)
            else:
                out = of.visualise_flow(fin, **kw)
            meta['error'] = None
            meta['returned'] = 'tensor' if isinstance(out, torch.Tensor) else 'ndarray'
            out = out.numpy() if isinstance(out, torch.Tensor) else out
        except Exception as exc:  # noqa: BLE001
            meta['error'] = [type(exc).__name__, str(exc)]
            out = np.zeros(0, np.uint8)
        meta['flow'] = put(flow)
        meta['mask'] = None if mask is None else put(mask)
        store['c%d_out' % k] = out
        store['c%d_meta' % k] = np.array(json.dumps(meta))
        k += 1

    n, h, w = 3, 19, 26
    flows = [smooth(n, h, w, 4.0), smooth(n, h, w, 0.02), rs.randn(n, 2, h, w).astype(np.float32) * 3]
    flows[2][:, :, 3:6, 4:9] = 0                                       # zero and near-threshold vectors
    flows[2][:, 0, 7, :] = np.float32(9.99e-4)
    flows[2][:, 1, 8, :] = np.float32(-1e-3)
    mask = rs.rand(n, h, w) > 0.25
    mask[:, 5:12, 6:15] = False
    for fi, fl in enumerate(flows):
        for mode in ('hsv', 'rgb', 'bgr'):
            for sm in (False, True):
                for sb in (False, True):
                    for rm in (None, 2.5, [1, 7.25, 0.5]):
                        if fi > 0 and not (rm is None or (sm == sb)):
                            continue
                        rec(fl, mask, mode=mode, show_mask=sm, show_mask_borders=sb, range_max=rm, return_tensor=False)
        rec(fl, mask, mode='bgr', show_mask=True, show_mask_borders=True)             # tensor N-3-H-W
        rec(fl, None, mode='rgb', show_mask=False, show_mask_borders=True)            # no mask: the 1-pixel frame
    # special flows: constant magnitude, all zero, a mask of 0 / 1 / 2 valid pixels, a width that is not a multiple of 4
    const = np.zeros((2, 2, 9, 11), np.float32)
    const[:, 0], const[:, 1] = 3.0, -4.0
    rec(const, None, mode='bgr', return_tensor=False)
    rec(np.zeros((2, 2, 9, 11), np.float32), None, mode='rgb', return_tensor=False)
    rec(np.zeros((2, 2, 9, 11), np.float32), None, mode='hsv', return_tensor=False)
    few = smooth(3, 9, 11, 2.0)
    fm = np.zeros((3, 9, 11), bool)
    fm[1, 4, 5] = True
    fm[2, 0, 0] = fm[2, 8, 10] = True
    rec(few[1:], fm[1:], mode='bgr', show_mask=True, return_tensor=False)
    rec(few[1:], fm[1:], mode='hsv', show_mask=True, show_mask_borders=True)
    rec(few, fm, mode='bgr', show_mask=True, return_tensor=False)                # IndexError
    rec(few, fm, mode='bgr', show_mask=False, return_tensor=False)
    # visualise_flow: 4-D and 3-D, tensor and array input
    f3 = smooth(1, 13, 17, 3.0)
    rec(f3, None, api='visualise_flow', mode='bgr')
    rec(f3[0], None, api='visualise_flow', mode='rgb', return_tensor=False)
    rec(f3[0], None, api='visualise_flow', tensor=False, mode='hsv', range_max=1.5)
    rec(np.moveaxis(f3[0], 0, -1).copy(), None, api='visualise_flow', tensor=False, mode='bgr')
    store['count'] = np.array(k)
    out = os.path.join(HERE, 'vis.npz')
    np.savez_compressed(out, **store)
    print("wrote", out, k, "cases,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
