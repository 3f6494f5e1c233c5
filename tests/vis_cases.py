"""The visualise fixtures (tests/golden/vis.npz, written by tests/golden/gen_visualise.py from the reference): loading them and
running one case through this package's API or through the oracle (tests/vis_oracle.py).  Shared by the CPU and GPU tiers."""
import json
import os

import numpy as np
import torch

import vis_oracle as vo

VIS_NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vis.npz')
_Z = None


def _z():
    global _Z
    if _Z is None:
        _Z = np.load(VIS_NPZ)
    return _Z


def case_ids():
    return list(range(int(_z()['count'])))


def case(k: int):
    """(meta dict, flow array, mask array or None, expected output array)"""
    z = _z()
    meta = json.loads(str(z['c%d_meta' % k]))
    mask = None if meta['mask'] is None else z[meta['mask']]
    return meta, z[meta['flow']], mask, z['c%d_out' % k]


def kwargs(meta):
    kw = {k: meta[k] for k in ('mode', 'show_mask', 'show_mask_borders', 'range_max', 'return_tensor') if k in meta}
    if meta['api'] == 'visualise_flow':
        kw.pop('show_mask', None)
        kw.pop('show_mask_borders', None)
    return kw


def run_api(ofl, meta, flow, mask, device):
    """The case through this package: (output or None, (exception type name, message) or None)"""
    fin = torch.from_numpy(flow).to(device) if meta['tensor'] else flow
    try:
        if meta['api'] == 'flow':
            out = ofl.Flow(fin, 't', None if mask is None else torch.from_numpy(mask).to(device)).visualise(**kwargs(meta))
        else:
            out = ofl.visualise_flow(fin, **kwargs(meta))
    except Exception as exc:  # noqa: BLE001
        return None, (type(exc).__name__, str(exc))
    return out, None


def as_nchw(flow: np.ndarray) -> np.ndarray:
    """N-2-H-W view of a fixture's flow input (visualise_flow also takes 2-H-W, H-W-2, N-H-W-2)"""
    f = flow if flow.ndim == 4 else flow[None]
    return f if f.shape[1] == 2 else np.moveaxis(f, -1, 1)


def run_oracle(meta, flow, mask):
    """The case through the oracle, in the reference's output layout: (output or None, error or None)"""
    f = as_nchw(flow).astype(np.float32)
    n = f.shape[0]
    rm = meta.get('range_max')
    rng = None if rm is None else np.broadcast_to(np.asarray(rm, np.float64), (n,))
    try:
        out = vo.visualise(f, meta['mode'], mask, meta.get('show_mask', False), meta.get('show_mask_borders', False), rng)
    except IndexError as exc:
        return None, (type(exc).__name__, str(exc))
    if meta['mode'] != 'hsv' and meta.get('return_tensor') is not False:
        out = np.moveaxis(out, -1, 1)
    if meta['api'] == 'visualise_flow' and flow.ndim == 3:
        out = out[0]
    return out, None
