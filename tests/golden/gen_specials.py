#!/usr/bin/env python3
"""Generate tests/golden/specials.npz by running the REFERENCE (oflibpytorch v2.1.1, PyTorch CPU) on images that carry NaN, +-inf,
denormals, -0.0 and FLT_MAX at the named positions of tests/special_values.py, 24 x 36.

Runs only where the reference's sources exist (like gen_golden.py and gen_visualise.py; `cv2` is not installed there and nothing on
this path calls it, so an empty stand-in module serves the import).  Inputs and outputs only; no other fixture file is touched.

    python tests/golden/gen_specials.py <path to the reference's src/>

Stored:  s_flow, s_data, s_mask, s_ca  (splat_case(24, 36, c=3, n=2, seed=0) and its first mask-channel mask)
         s_apply_flow_masked / s_apply_flow_unmasked          apply_flow(flow, data, 's', mask | None)
         s_no_occlusion, s_no_occlusion_density               apply_s_flow(flow, data, mask, occlude_zero_flow=False)
         s_flow_apply, s_flow_apply_valid                     Flow(flow, 's', mask).apply(data, ca, return_valid_area=True)
         t_flow, t_src, t_mask, t_tmask  (warp_case(2, 24, 36, 3, seed=0), a flow mask and a target mask)
         t_apply_flow                                         apply_flow(flow, src, 't')
         t_flow_apply, t_flow_apply_valid                     Flow(flow, 't', mask).apply(src, tmask, return_valid_area=True)
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import special_values as sv  # noqa: E402

H, W = 24, 36


def main():
    if len(sys.argv) < 2:
        sys.exit("usage: gen_specials.py <path to the reference's src/>")
    src = sys.argv[1]
    sys.modules.setdefault('cv2', types.ModuleType('cv2'))
    sys.path.insert(0, src)
    import oflibpytorch as of
    from oflibpytorch import utils as ofu
    warnings.simplefilter("ignore")
    tt = torch.from_numpy
    store = {}

    s = sv.splat_case(H, W, c=3, n=2, seed=0)
    flow, data, mask, ca = s["flow"], s["data"], s["mask"], s["ca"]
    store.update(s_flow=flow, s_data=data, s_mask=mask, s_ca=ca)
    store["s_apply_flow_masked"] = ofu.apply_flow(tt(flow), tt(data), 's', tt(mask)).numpy()
    store["s_apply_flow_unmasked"] = ofu.apply_flow(tt(flow), tt(data), 's').numpy()
    out, dens = ofu.apply_s_flow(tt(flow), tt(data), tt(mask), occlude_zero_flow=False)
    store["s_no_occlusion"], store["s_no_occlusion_density"] = out.numpy(), dens.numpy()
    out, valid = of.Flow(tt(flow), 's', tt(mask)).apply(tt(data), tt(ca), return_valid_area=True)
    store["s_flow_apply"], store["s_flow_apply_valid"] = out.numpy(), valid.numpy()

    t = sv.warp_case(2, H, W, 3, seed=0)
    rng = np.random.default_rng(5)
    fmask, tmask = rng.random((2, H, W)) > 0.1, rng.random((2, H, W)) > 0.1
    store.update(t_flow=t["flow"], t_src=t["src"], t_mask=fmask, t_tmask=tmask)
    store["t_apply_flow"] = ofu.apply_flow(tt(t["flow"]), tt(t["src"]), 't').numpy()
    out, valid = of.Flow(tt(t["flow"]), 't', tt(fmask)).apply(tt(t["src"]), tt(tmask), return_valid_area=True)
    store["t_flow_apply"], store["t_flow_apply_valid"] = out.numpy(), valid.numpy()

    path = os.path.join(HERE, 'specials.npz')
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
