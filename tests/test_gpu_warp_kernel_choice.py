"""GPU tier: WHICH kernel the fp32, uint8, fp16-source and gradient entry points of the backward warp launch, per size class of the
launch and per OFL_OPT_WARP_PATH value -- and that the launch computes what a second route computes, bit for bit.

tests/test_gpu_half_warp.py pins the choice of the 16-bit entry point (ofl_warp_bwd_x16) and tests/test_gpu_half_warp_backward.py
that of its gradient; this file pins the others.  Every case is ONE `_native` call.  Afterwards `_native.last_kernel_name()` must be
the string recorded for the case in tests/golden/warp_kernel_choice.json (recorded with tools/record_warp_kernel_choice.py at the
commit BEFORE the launchers were rewritten around warp_choose(), never from the code under test), and the results must equal
(torch.equal) those of a second route: for the fp32 kinds the same call under set_warp_path(1), the generic kernels; for the uint8
and fp16-source kinds the fp32 entry point on the converted source (as the path loops of tests/test_gpu_parity.py do).

The launcher's thresholds count tiles of the 32-wide geometry -- g1: 32 x 16 tiles, g4: groups of four of them, 32 x 64 -- over the
whole batch, rounded up to a multiple of 8.  So batches of tiny frames cross them with a few megabytes of data: a 16 x 32 frame is
one tile and one group (g1 = g4 = n), lean (W % 4 == 0); 16 x 30 the same but not lean; 64 x 30 four tiles and one group, which
reaches the pair kernel (g1 >= kColumnMinGroups > g4); 8 x 16 frames feed the channel loop.  The batch sizes are DERIVED from the
constants of ofl_kernels.hip (OFL_ROWS_T1_MAX, OFL_ROWS_T4_MIN, kColumnMinGroups, OFL_WARP_CHAN_WIDE_MIN, read from the source
below), one batch on either side of each; the ids carry them, so a changed threshold shows as ids missing from the table."""
import json
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, 'tests', 'golden', 'warp_kernel_choice.json')
PATHS = (0, 3, 4, 5, 6, 7)


def _constants():
    """The launcher's thresholds, from the source that defines them."""
    with open(os.path.join(ROOT, 'oflibpytorch_amd', 'csrc', 'ofl_kernels.hip')) as fh:
        text = fh.read()
    col = int(re.search(r"constexpr unsigned kColumnMinGroups = (\d+)", text).group(1))

    def macro(name):
        body = re.search(r"^#define %s +(\(.*?\)|\S+)" % name, text, re.M).group(1)
        body = re.sub(r"(\d+)u\b", r"\1", body).replace("kColumnMinGroups", str(col))
        assert re.fullmatch(r"[\d\s()*+]+", body), body
        return int(eval(body))

    return dict(t1=macro("OFL_ROWS_T1_MAX"), t4=macro("OFL_ROWS_T4_MIN"), col=col, chan=macro("OFL_WARP_CHAN_WIDE_MIN"))


def _sides(threshold, per_frame=1):
    """Batch sizes just below and at a threshold on a tile count that is `per_frame` tiles per image, rounded up to 8."""
    at = -(-threshold // (8 * per_frame)) * 8
    return at - 8, at


def cases():
    """Every case of this file as a dict with a stable `id` (also what tools/record_warp_kernel_choice.py walks)."""
    k = _constants()
    (t1_lo, t1), (t4_lo, t4), (col_lo, col) = _sides(k["t1"]), _sides(k["t4"]), _sides(k["col"])
    every = (t1_lo, t1, t4_lo, t4, col_lo, col)
    lean, ragged, tall, tiny = (16, 32), (16, 30), (64, 30), (8, 16)
    out = []

    def add(kind, frame, n, c, path, **kw):
        tag = "".join("-%s%s" % (key, "" if val is True else val) for key, val in sorted(kw.items()) if val not in (None, False))
        out.append(dict(id="%s-%dx%d-n%d-c%d%s-p%d" % (kind, frame[0], frame[1], n, c, tag, path), kind=kind, h=frame[0], w=frame[1], n=n,
                        c=c, path=path, **kw))

    # a plain warp, 1 ... 3 channels, with and without the valid area
    for c in (1, 2, 3):
        for valid in (False, True):
            for n in every:
                add("plain", lean, n, c, 0, valid=valid)
            for n in (t1_lo, col_lo, col):
                add("plain", ragged, n, c, 0, valid=valid)
                for path in PATHS[1:]:
                    add("plain", lean, n, c, path, valid=valid)
            for path in PATHS:
                add("plain", tall, _sides(k["col"], 4)[1], c, path, valid=valid)
            for n in (col_lo, col):
                for path in PATHS[1:]:
                    add("plain", ragged, n, c, path, valid=valid)
    # an addend: the flow itself (mode 3 proper), another field; 2 channels is where the fused kernels are, 1 and 3 fall through
    for valid in (False, True):
        for n in every:
            add("plain", lean, n, 2, 0, valid=valid, addend="flow")
        for n in (t4_lo, t4, col_lo, col):
            add("plain", lean, n, 2, 0, valid=valid, addend="other")
        for n in (col_lo, col):
            for addend in ("flow", "other"):
                add("plain", ragged, n, 2, 0, valid=valid, addend=addend)
        for path in PATHS[1:]:
            for addend in ("flow", "other"):
                add("plain", lean, col, 2, path, valid=valid, addend=addend)
                add("plain", lean, t1_lo, 2, path, valid=valid, addend=addend)
            add("plain", ragged, col, 2, path, valid=valid, addend="flow")
    for c in (1, 3):
        for n in (col_lo, col):
            add("plain", lean, n, c, 0, valid=True, addend="other")
    # src - src_b formed in the kernel, the flag word of the output, the flag words of the flow (and of the source)
    for path in PATHS:
        for frame in (lean, ragged):
            for n in (col_lo, col):
                add("plain", frame, n, 2, path, valid=True, src_b=True)
                add("plain", frame, n, 2, path, valid=True, dst_flags=True)
        for n in (col_lo, col):
            add("plain", lean, n, 2, path, valid=True, flags=True)
        add("plain", lean, col, 2, path, valid=True, flags="src")
    for path in (0, 6):
        for addend in ("flow", "other"):
            for frame in (lean, ragged):
                for n in (col_lo, col):
                    add("plain", frame, n, 2, path, valid=True, dst_flags=True, addend=addend)
    add("plain", lean, col, 2, 0, valid=True, flags=True, addend="flow")
    # a uint8 source with uint8 and with fp32 output
    for c in (1, 3):
        for to_u8 in (False, True):
            for valid in (False, True):
                for n in (col_lo, col):
                    add("u8", lean, n, c, 0, valid=valid, to_u8=to_u8)
            for path in PATHS[1:]:
                add("u8", lean, col, c, path, valid=True, to_u8=to_u8)
            add("u8", ragged, col, c, 0, valid=True, to_u8=to_u8)
    add("u8", lean, col, 2, 0, valid=True, to_u8=True)
    # an fp16 source (a flow stored in halves) with and without src_b
    for src_b in (False, True):
        for n in (col_lo, col):
            for path in PATHS:
                add("half", lean, n, 2, path, valid=True, src_b=src_b)
        add("half", ragged, col, 2, 0, valid=True, src_b=src_b)
        add("half", ragged, col_lo, 2, 0, valid=True, src_b=src_b)
    # the gradient with respect to the flow
    for c in (1, 2, 3):
        for n in every:
            add("grad", lean, n, c, 0)
        for n in (col_lo, col):
            add("grad", ragged, n, c, 0)
            for path in PATHS[1:]:
                add("grad", lean, n, c, path)
    # more than 3 channels: the channel loop (from 7 channels on with the valid area), on either side of OFL_WARP_CHAN_WIDE_MIN
    chan_lo, chan = _sides(k["chan"])
    for valid in (False, True):
        for c in (4, 6, 7, 8):
            for path in (0, 5, 6):
                add("plain", tiny, 8, c, path, valid=valid)
        for n in (chan_lo, chan):
            add("plain", tiny, n, 4, 0, valid=valid)
            add("plain", tiny, n, 4, 0, valid=valid, flags=True)
            add("plain", tiny, n, 8, 6, valid=valid)
    return out


CASES = cases()
with open(TABLE) as _fh:
    RECORDED = json.load(_fh)
_DATA, _SECOND, _NAMES = {}, {}, {}


def _data(case, dev):
    """flow, source planes (fp32 / uint8 / fp16), another field, masks for the case's batch of frames (cached per shape)."""
    key = (case["n"], case["h"], case["w"])
    if key not in _DATA:
        n, h, w = key
        g = torch.Generator(device=dev).manual_seed(n + 31 * h + w)
        flow = torch.randn(n, 2, h, w, generator=g, device=dev) * 2.5
        flow[:, :, :3, :3] = 40.0                         # (taps that leave the frame)
        planes = torch.rand(n, 8, h, w, generator=g, device=dev) * 255
        other = torch.randn(n, 3, h, w, generator=g, device=dev)
        mask = torch.rand(n, h, w, generator=g, device=dev) > 0.15
        if len(_DATA) >= 3:
            _DATA.pop(next(iter(_DATA)))
        _DATA[key] = (flow, planes, other, mask)
    return _DATA[key]


def _call(case, dev, second=False):
    """The case's one `_native` call (second: the route it is compared with); the results that are tensors."""
    from oflibpytorch_amd import _native
    flow, planes, other, mask = _data(case, dev)
    c, kind = case["c"], case["kind"]
    src = planes[:, :c].contiguous() if c != 8 else planes
    kw = {}
    if case.get("valid"):
        kw.update(want_valid=True, src_mask=mask, flow_mask=mask)
    if kind == "grad":
        gout = (planes[:, 8 - c:] - 100).contiguous()
        return _native.warp_bwd_grad(flow, src, gout, g_scale=0.5, want_src=False)[1:]
    if case.get("addend"):
        kw.update(addend=flow if case["addend"] == "flow" else other[:, :c].contiguous(), a_sign=1.0, g_sign=-1.0)
    if case.get("dst_flags"):
        kw.update(want_dst_flags=True)
    if case.get("flags"):
        kw.update(want_flags=True, want_src_flags=case["flags"] == "src")
    b = (other[:, :2] * 30).contiguous() if case.get("src_b") else None
    if kind == "plain":
        return _native.warp_bwd(flow, src, src_b=b, **kw)
    if kind == "half":
        return _native.warp_bwd(flow, (src / 16).half() if not second else (src / 16).half().float(), src_b=b, **kw)
    assert kind == "u8"
    rm = _native.ROUND_U8 if case.get("to_u8") else _native.ROUND_NONE
    if not second:
        return _native.warp_bwd(flow, src.to(torch.uint8), round_mode=rm, out_uint8=bool(case.get("to_u8")), **kw)
    res = _native.warp_bwd(flow, src.to(torch.uint8).float(), round_mode=rm, **kw)
    return (res[0].to(torch.uint8) if case.get("to_u8") else res[0],) + tuple(res[1:])


def run_case(case, dev):
    """(results, demangled name of the kernel launched last) of the case under its path option."""
    from oflibpytorch_amd import _native
    _native.set_warp_path(case["path"])
    try:
        res = _call(case, dev)
        raw = _native.last_kernel_name(demangle=False)
        if raw not in _NAMES:
            _NAMES[raw] = _native.last_kernel_name()
    finally:
        _native.set_warp_path(0)
    return res, _NAMES[raw]


def _second_route(case, dev):
    """The case's results by its second route (the same for every path option: cached without it)."""
    from oflibpytorch_amd import _native
    key = case["id"].rsplit("-p", 1)[0]
    if key not in _SECOND:
        if len(_SECOND) >= 4:
            _SECOND.pop(next(iter(_SECOND)))
        _native.set_warp_path(1 if case["kind"] in ("plain", "grad") else 0)
        try:
            _SECOND[key] = _call(case, dev, second=True)
        finally:
            _native.set_warp_path(0)
    return _SECOND[key]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tier needs a HIP device"
    from oflibpytorch_amd import _native
    _native.load_library()
    return torch.device('cuda', 0)


def test_case_ids_are_unique_and_recorded():
    ids = [c["id"] for c in CASES]
    assert len(set(ids)) == len(ids)
    assert set(ids) == set(RECORDED), sorted(set(ids) ^ set(RECORDED))[:10]


@pytest.mark.parametrize("case", sorted(CASES, key=lambda c: (c["n"], c["h"], c["w"], c["id"].rsplit("-p", 1)[0])), ids=lambda c: c["id"])
def test_the_recorded_kernel_runs_and_equals_the_second_route(case, dev):
    got, name = run_case(case, dev)
    assert name == RECORDED[case["id"]]
    ref = _second_route(case, dev)
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.dtype == b.dtype and torch.equal(a, b)
