"""NumPy oracle of Flow.consistency / consistency_mask / filter_consistent, written from DESIGN.md 3.18 (a helper module, not a test).

The partner (bu, bv) and the weight test mr > 0.99999 come from `oracle_backend.warp_bwd` (the C oracle of the backward warp, which the
reference pins); everything after it is elementwise np.float32 arithmetic, one rounding per operation; the records come from math.fsum.
Also here: the inputs the CPU and the GPU tier share (`case`), the categories a pixel can fall into (`categories`), and a stand-in for
`_consistency.flow_consistency` for the host-logic tests (`fake_flow_consistency`)."""
import functools

import numpy as np
import torch

import oracle_backend as ob
import special_values as sv

ALPHA, BETA = 0.01, 0.5
# (n, h, w): the frames of the GPU tier (tests/test_gpu_consistency.py says what each exercises)
FRAMES = [(1, 2, 2), (2, 5, 7), (3, 8, 12), (2, 20, 28), (2, 67, 131), (1, 1080, 1920)]
# (alpha, beta) of the table.  The API's defaults (0.01, 0.5) are tested on their own; the table runs with beta = 0.1 because the noise
# below reaches a partner blended over four taps (about 0.55 of its amplitude), of which the default bound lets most pass in the small
# frames; the vectors of the 1080p case reach 60 px, where alpha = 0.01 alone puts the bound over 40 px^2, beyond any noise of +-2 px:
# that frame runs with a smaller alpha.  test_consistency_host.py checks that every frame of 8 x 8 and more shows every category
TABLE_BETA = 0.1
FRAME_ALPHA = {(1, 1080, 1920): 1.0e-4}


def check(a, back, a_mask=None, back_mask=None, ref='s', alpha=ALPHA, beta=BETA):
    """a, back [N,2,H,W] float32 (or float16: up-converted exactly), masks [N,H,W] bool or None (all True: `consider_mask=False`).
    Returns a dict: 'du', 'dv' float32 and 'known' bool (the vectors and the mask of combine_with mode 3), 'error' float32 (0 where not
    known), 'consistent' bool, 'records' float64 [N,8]."""
    a = np.asarray(a).astype(np.float32)
    back = np.asarray(back).astype(np.float32)
    n = a.shape[0]
    sign = -1.0 if ref == 's' else 1.0
    out, valid, _, _ = ob.warp_bwd(torch.from_numpy(a.copy()), torch.from_numpy(back.copy()), flow_sign=sign,
                                   src_mask=None if back_mask is None else torch.from_numpy(np.array(back_mask, bool)), want_valid=True)
    out = out.numpy()
    u, v, bu, bv = a[:, 0], a[:, 1], out[:, 0], out[:, 1]
    known = valid.numpy().astype(bool)
    if a_mask is not None:
        known = known & np.asarray(a_mask, bool)
    al, be = np.float32(alpha), np.float32(beta)
    with np.errstate(all='ignore'):
        du, dv = u + bu, v + bv
        e2 = du * du + dv * dv
        e = np.sqrt(e2)
        m2 = (u * u + v * v) + (bu * bu + bv * bv)
        bound = al * m2 + be
        consistent = known & (e2 <= bound)
    assert du.dtype == np.float32 and e.dtype == np.float32 and bound.dtype == np.float32
    error = np.where(known, e, np.float32(0.0)).astype(np.float32)
    rec = np.zeros((n, 8), np.float64)
    for i in range(n):
        ek, ec = e[i][known[i]].astype(np.float64), e[i][consistent[i]].astype(np.float64)
        rec[i, :5] = [ek.size, ec.size, sv.record_sum(ek), sv.record_max(ek), sv.record_sum(ec)]
    return {'du': du, 'dv': dv, 'known': known, 'error': error, 'consistent': consistent, 'records': rec}


@functools.lru_cache(maxsize=None)
def case(n, h, w, ref, scale=1.0):
    """(a, back, a_mask, back_mask) as read-only NumPy arrays, seeds fixed (`scale` multiplies `a`: at 0.1 the partners of a frame of
    2 x 2 or 5 x 7 stay inside it, which the translation below leaves almost everywhere).  `a`: the translation (3.3, -2.6) plus an affine field
    whose four partial derivatives are 0.02 per pixel in size, signed so that the partners of the pixels along two edges leave the
    frame whichever way the reference makes them go.  `back` = -a plus uniform noise of +-2 px on the middle third of the columns (a
    band that the partners of known pixels reach in the smallest frames too, for both references).  Both masks random with 20 % holes,
    the holes square cells of max(2, min(h, w) // 8) pixels (single-pixel holes would leave the four taps of a partner all valid at
    0.8^4 = 41 % of the pixels only, too few to show both kinds of known pixel in a frame of 8 x 12)."""
    rs = np.random.RandomState(7919 * n + 31 * h + w + (0 if ref == 's' else 500000))
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    g, s = 0.02, (1.0 if ref == 's' else -1.0)
    a = np.empty((n, 2, h, w), np.float32)
    for i in range(n):
        k = 1.0 - 0.1 * i                                    # (the images of a batch differ)
        a[i, 0] = scale * (3.3 + s * k * g * (x + y))
        a[i, 1] = scale * (-2.6 - s * k * g * ((h - 1 - y) + (w - 1 - x)))
    back = -a
    noise = (rs.rand(n, 2, h, w) * 4.0 - 2.0).astype(np.float32)
    band = slice(w // 3, (2 * w + 2) // 3)
    back[:, :, :, band] += noise[:, :, :, band]
    cell = max(2, min(h, w) // 8)

    def holes():
        cells = rs.rand(n, (h + cell - 1) // cell, (w + cell - 1) // cell) > 0.2
        return np.ascontiguousarray(np.repeat(np.repeat(cells, cell, 1), cell, 2)[:, :h, :w])

    am, bm = holes(), holes()
    for arr in (a, back, am, bm):
        arr.setflags(write=False)
    return a, back, am, bm


def frame_params(n, h, w):
    """(alpha, beta) of a frame of the table"""
    return FRAME_ALPHA.get((n, h, w), ALPHA), TABLE_BETA


@functools.lru_cache(maxsize=None)
def reference(n, h, w, ref, masked=True, scale=1.0):
    """The oracle's result for `case(n, h, w, ref, scale)`, computed once and shared (treat as read-only)."""
    a, back, am, bm = case(n, h, w, ref, scale)
    return check(a, back, am if masked else None, bm if masked else None, ref, *frame_params(n, h, w))


def categories(n, h, w, ref):
    """The share of the pixels of a case in each of the four categories: known and consistent, known and inconsistent, unknown
    because the partner leaves the frame, unknown because of a mask (known without the masks, not with them)."""
    with_masks, without = reference(n, h, w, ref), reference(n, h, w, ref, False)
    total = float(n * h * w)
    return {'consistent': (with_masks['known'] & with_masks['consistent']).sum() / total,
            'inconsistent': (with_masks['known'] & ~with_masks['consistent']).sum() / total,
            'leaves_frame': (~without['known']).sum() / total,
            'masked': (without['known'] & ~with_masks['known']).sum() / total}


def fake_flow_consistency(a, back, a_mask=None, back_mask=None, flow_sign=-1.0, alpha=ALPHA, beta=BETA, want_error=True,
                          want_consistent=True, want_known=True, want_record=True):
    """`_consistency.flow_consistency` served by the oracle on the CPU (host-logic tests)."""
    r = check(a.detach().numpy(), back.detach().numpy(), None if a_mask is None else a_mask.numpy(),
              None if back_mask is None else back_mask.numpy(), 's' if flow_sign < 0 else 't', alpha, beta)
    return (torch.from_numpy(r['error']) if want_error else None, torch.from_numpy(r['consistent']) if want_consistent else None,
            torch.from_numpy(r['known']) if want_known else None, torch.from_numpy(r['records']) if want_record else None)
