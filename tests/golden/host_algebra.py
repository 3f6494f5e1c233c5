#!/usr/bin/env python3
"""The 3 x 3 matrices that HOST linear algebra forms on the way to a generated field -- `torch.pinverse` (from_matrix 't',
utils.py:702) and the product of transform matrices (`matrix_from_transforms`, utils.py:379-393) -- as the fixtures' host formed
them, per golden case, in call order: tests/golden/host_algebra.npz.

MKL / LAPACK choose their kernels by CPU model, so those nine numbers can differ in the last bit from one host to another (the
reference itself would differ the same way), and every value of the field after them with it.  The CPU tier
(tests/test_host_logic_golden.py) replays the recorded matrices through `pin`: each call still runs, its result must agree with the
recorded one to fp32 rounding, and the recorded one goes on -- so the field is held to the reference's fixture bit for bit on
any host.

    python tests/golden/host_algebra.py

re-records them on a host where every CPU-tier case meets its fixture bit for bit with its OWN linear algebra (it refuses to
write otherwise)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "host_algebra.npz")
_records = None


def _load():
    global _records
    if _records is None:
        _records = {}
        with np.load(PATH) as z:
            for key in sorted(z.files, key=lambda k: (k.split("|")[0], int(k.split("|")[1]))):
                cid, _, kind = key.split("|")
                _records.setdefault(cid, []).append((kind, z[key]))
    return _records


def _targets():
    from oflibpytorch_amd import utils
    return ((torch, "pinverse"), (utils, "matrix_from_transforms"))


def pin(cid, monkeypatch):
    """Replay case `cid`'s recorded matrices (nothing to do for a case without any).  -> a function that asserts, after the
    case, that every recorded matrix was asked for."""
    queue = list(_load().get(cid, ()))
    if not queue:
        return lambda: None

    def wrap(kind, real):
        def replay(*args, **kwargs):
            got = real(*args, **kwargs)
            assert queue, "%s: more %s calls than recorded" % (cid, kind)
            k, want = queue.pop(0)
            assert k == kind, "%s: %s called where %s was recorded" % (cid, kind, k)
            want = torch.from_numpy(want).to(dtype=got.dtype, device=got.device)
            assert want.shape == got.shape, (cid, kind, tuple(want.shape), tuple(got.shape))
            scale = max(float(want.abs().max()), 1.0)
            torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5 * scale, msg="%s: this host's %s" % (cid, kind))
            return want
        return replay
    for mod, name in _targets():
        monkeypatch.setattr(mod, name, wrap(name, getattr(mod, name)))

    def done():
        assert not queue, "%s: %d recorded matrices never asked for" % (cid, len(queue))
    return done


def record():
    import pytest
    sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]
    import case_runner
    import oracle_backend
    from conftest import _GOLDEN as golden
    from oflibpytorch_amd import _native
    from test_host_logic_golden import ALL
    routed = ("flow_flags", "warp_bwd", "splat_fwd", "device", "sample_pts", "flow_extents", "warp_bwd_win", "splat_fwd_win",
              "_wants_grad", "flow_from_matrix", "warp_valid")          # (what conftest.oracle_native routes to the oracle)
    out = {}
    for cid in ALL:
        seen = []
        with pytest.MonkeyPatch.context() as mp:
            for name in routed:
                mp.setattr(_native, name, getattr(oracle_backend, name))
            for mod, name in _targets():
                def rec(*args, _real=getattr(mod, name), _kind=name, **kwargs):
                    r = _real(*args, **kwargs)
                    seen.append((_kind, r.detach().cpu().numpy().copy()))
                    return r
                mp.setattr(mod, name, rec)
            case = golden.cases[cid]
            case_runner.check_case(case, golden, case_runner.run_case(case, golden, torch.device('cpu')), exact_values=True)
        for i, (kind, a) in enumerate(seen):
            out["%s|%d|%s" % (cid, i, kind)] = a
    np.savez_compressed(PATH, **out)
    print("%s: %d matrices of %d cases" % (PATH, len(out), len({k.split("|")[0] for k in out})))


if __name__ == "__main__":
    record()
