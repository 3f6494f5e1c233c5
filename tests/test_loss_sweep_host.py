"""CPU tier of the loss sweep (tests/frame_sweep.py, tests/loss_sweep.py): what keeps
tests/test_gpu_loss_sweep_*.py and the gradient tests of tests/test_gpu_frame_sweep_stream.py from passing vacuously, proved from the
constants read out of the sources -- no GPU.  Every condition is an assertion; nothing is skipped."""
import numpy as np
import pytest
import torch

import census_oracle as cen
import frame_sweep as fs
import loss_sweep as ls
import photometric_oracle as po
import smoothness_oracle as so

G = fs.loss_geometry()
LOOPS = fs.loop_frames()
CPU = torch.device('cpu')


# ---- geometry and frames ----------------------------------------------------------------------------------------------------------------
def test_the_geometry_is_todays():
    """A changed constant fails here first: the frames of `loop_frames()` follow it, but someone has to look at them."""
    assert G == {"smoothness": {"kTH": 8, "kTW": 128, "kMaxBlocks": 256, "kMaxGradBlocks": 1024},
                 "census": {"kTileW": 64, "kTileH": 16, "kChunk": 256},
                 "photometric": {"kThreads": 256, "kMaxBlocks": 256, "kMaxGradBlocks": 2048},
                 "metrics": {"kThreads": 256, "kMaxBlocks": 256, "kMaxGradBlocks": 2048, "grad_pixels": 4}}
    assert LOOPS == {
        "photometric_fwd": [("partial_second_round", 257, 257), ("step_x_zero", 129, 512), ("second_row", 2, 32771),
                            ("step_y_zero", 2, 65539), ("step_x_zero", 258, 256), ("three_rounds", 3, 43700)],
        "photometric_bwd": [("partial_second_round", 725, 725), ("step_x_zero", 1025, 512), ("second_row", 2, 262147),
                            ("step_y_zero", 2, 524291)],
        "smoothness_fwd": [("ragged_scalar", 1033, 129), ("ragged_vector", 1033, 132), ("three_rounds", 1361, 260)],
        "smoothness_bwd": [("ragged_scalar", 4105, 129), ("ragged_vector", 4105, 132), ("three_rounds", 5457, 260)],
        "census_finish": [("one_full_chunk", 32, 8192), ("full_chunk_and_two", 25, 8193), ("two_full_chunks", 32, 16384),
                          ("three_chunks", 41, 10881)],
        "epe_grad": [("second_round", 2, 1048579)]}


def test_the_frame_lists():
    assert len(fs.LOSS_TILE_FRAMES) == len(fs.FRAMES) + 10 == 176 and set(fs.FRAMES) < set(fs.LOSS_TILE_FRAMES)
    assert [f for f in fs.LOSS_TILE_FRAMES if f not in fs.FRAMES] == [(17, w) for w in range(252, 262)]
    assert min(min(f) for f in fs.LOSS_TILE_FRAMES) == 2 and fs.SMOOTHNESS_ONLY == [(1, 5), (5, 1), (1, 1)]
    e = G["photometric"]["kThreads"]
    sizes = fs.photo_sizes()
    hw = {h * w for h, w in sizes}
    assert hw >= {v for v in range(4, e + 9) if v % 2 == 0 or (v % 3 == 0 and v >= 6)} and min(min(s) for s in sizes) >= 2
    assert {v for k in (2, 3) for v in range(k * e - 3, k * e + 6) if v % 2 == 0 or v % 3 == 0} <= hw
    assert {w % 4 for h, w in sizes if h == 2} == {0, 1, 2, 3} == {w % 4 for h, w in sizes if h == 3}
    # the streaming sweep's sizes for the backward of the scores: its own E
    e = G["metrics"]["kThreads"] * G["metrics"]["grad_pixels"]
    assert {h * w for h, w in fs.stream_sizes(e)} >= {e - 2, e, e + 2, 2 * e - 2, 2 * e, 2 * e + 2, 3 * e - 3, 3 * e, 3 * e + 3}


def test_only_smoothness_takes_a_frame_of_one_row_or_column():
    """The C ABI's size checks come before any device call: photometric and census refuse H or W < 2, smoothness takes them."""
    from oflibpytorch_amd import _census, _photometric, _smoothness
    for h, w in fs.SMOOTHNESS_ONLY:
        assert _photometric._library().ofl_flow_photometric_workspace_bytes(4, h, w) < 0, (h, w)
        assert _smoothness._library().ofl_flow_smoothness_workspace_bytes(4, h, w) == 4 * 8 * 8, (h, w)
        for patch in fs.CENSUS_PATCHES:
            assert _census._library().ofl_flow_census_workspace_bytes(4, h, w, patch) < 0, (h, w)
    assert _photometric._library().ofl_flow_photometric_workspace_bytes(4, 2, 2) > 0
    assert _census._library().ofl_flow_census_workspace_bytes(4, 2, 2, 3) > 0


# ---- residues ---------------------------------------------------------------------------------------------------------------------------
def _residues(frames, tw, th, what, widths=None):
    ws, hs = {w for _, w in frames}, {h for h, _ in frames}
    for r in (widths or (0, 1, tw - 1)):
        assert any(w % tw == r for w in ws), "%s: no frame with W %% %d == %d" % (what, tw, r)
    for r in (0, 1, th - 1):
        assert any(h % th == r for h in hs), "%s: no frame with H %% %d == %d" % (what, th, r)
    assert any(w >= 2 * tw + 1 for w in ws) and any(h >= 2 * th + 1 for h in hs), "%s: no tile with a neighbour on both sides" % what


def test_every_smoothness_instantiation_meets_the_residues_of_its_tile():
    th, tw = G["smoothness"]["kTH"], G["smoothness"]["kTW"]
    frames = fs.LOSS_TILE_FRAMES + fs.SMOOTHNESS_ONLY
    for j, kind in enumerate(fs.SMOOTHNESS_KINDS):
        mine = [(h, w, fs.smoothness_variants(h, w)[j]) for h, w in frames]
        assert all((v["order"], v["kind"]) == kind for _, _, v in mine)
        scalar = [(h, w) for h, w, _ in mine if w % 4]
        vector = [(h, w) for h, w, _ in mine if w % 4 == 0]
        _residues(scalar, tw, th, "%s, scalar form" % (kind,), (1, tw - 1))
        _residues(vector, tw, th, "%s, 16-byte form" % (kind,), (0, 4, tw - 4))
        assert {w % 4 for _, w in scalar} == {1, 2, 3}
        assert any(h % th == th - 1 and h > th for h, _ in scalar) and any(h % th == th - 1 and h > th for h, _ in vector)      # 8 k - 1
        # what is no template argument takes both values in both forms, and at a ragged tile edge
        for form in (scalar, vector):
            for key in ("half", "masked"):
                for val in (False, True):
                    got = [(h, w) for h, w, v in mine if v[key] == val and (h, w) in form]
                    assert any(w > tw and w % tw for _, w in got) and any(h > th and h % th for h, _ in got), (kind, key, val)


def test_every_photometric_instantiation_meets_every_size():
    frames = fs.LOSS_TILE_FRAMES + fs.photo_sizes()
    for j, (half, u8) in enumerate(fs.TYPES):
        mine = [fs.photometric_variants(h, w)[j] for h, w in frames]
        assert all((v["half"], v["u8"]) == (half, u8) for v in mine)
        for lst in (fs.LOSS_TILE_FRAMES, fs.photo_sizes()):
            seen = {(v["ref"], v["chan"], v["masked"]) for v in (fs.photometric_variants(h, w)[j] for h, w in lst)}
            assert seen == {(r, c, m) for r in 'st' for c in (3, 1) for m in (False, True)}, (half, u8)


def test_every_census_instantiation_meets_the_residues_of_its_tile_and_the_halo():
    tw, th = G["census"]["kTileW"], G["census"]["kTileH"]
    for patch in fs.CENSUS_PATCHES:
        r = patch // 2
        for half, u8 in fs.TYPES:
            mine = [(h, w, v) for h, w in fs.LOSS_TILE_FRAMES for v in fs.census_variants(h, w)
                    if (v["patch"], v["half"], v["u8"]) == (patch, half, u8)]
            frames = [(h, w) for h, w, _ in mine]
            what = "patch %d half %s u8 %s" % (patch, half, u8)
            _residues(frames, tw, th, what)
            assert {w % 4 for _, w in frames} == {0, 1, 2, 3}, what
            # the backward's halo of 2 R against frames no wider / no taller than it (narrower where the family takes such a frame:
            # W, H >= 2, so at patch 3 the frame of 2 is the halo itself), and against last tiles of one column / one row
            assert any(w < max(2 * r, 3) for _, w in frames) and any(h < max(2 * r, 3) for h, _ in frames), what
            assert any(w <= r for _, w in frames) or r == 1, what
            assert any(w % tw == 1 and w > tw for _, w in frames) and any(h % th == 1 and h > th for h, _ in frames), what
            for key, vals in (("ref", 'st'), ("chan", (3, 1)), ("masked", (False, True)), ("q1", (False, True))):
                for val in vals:
                    got = [(h, w) for h, w, v in mine if v[key] == val]
                    assert any(w > tw and w % tw for _, w in got) and any(h > th and h % th for h, _ in got), (what, key, val)
    assert all(len(fs.census_variants(h, w)) in (4, 12) for h, w in fs.LOSS_TILE_FRAMES)


# ---- loop states ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_the_photometric_loop_frames_reach_their_states(backward):
    """The carried (x, y) equals divmod(pix, w) at every pixel of every loop frame (asserted inside the walk), each frame is in the
    state it is listed for, both branches of the wrap test are taken, and x + step_x == w occurs."""
    frames = LOOPS["photometric_bwd" if backward else "photometric_fwd"]
    stride = G["photometric"]["kMaxGradBlocks" if backward else "kMaxBlocks"] * G["photometric"]["kThreads"]
    states, exact = set(), 0
    for state, h, w in frames:
        walk = fs.photometric_walk(h, w, backward)
        print(state, h, w, walk)
        assert h * w > stride and walk["rounds"] >= 2, (state, h, w)
        if state == "partial_second_round":
            assert walk["rounds"] == 2 and walk["step_x"] > 0 and walk["step_y"] > 0 and walk["wraps"] > 0 and walk["straight"] > 0
            assert walk["first_round_wrap"]                                 # the wrap is taken by the first carry of a lane
            assert h % 2 == 1 and w % 2 == 1
        elif state == "step_x_zero":
            assert walk["step_x"] == 0 and walk["step_y"] > 0 and walk["wraps"] == 0 and walk["straight"] > 0
        elif state == "step_y_zero":
            assert walk["step_y"] == 0 and walk["step_x"] == stride and w > stride and walk["wraps"] > 0
        elif state == "second_row":
            assert walk["rounds"] == 2 and walk["step_y"] == 1 and walk["wraps"] == 0 and walk["straight"] == h * w - stride      # row 0 to row 1
        else:
            assert state == "three_rounds" and walk["rounds"] == 3 and walk["wraps"] > 0 and walk["straight"] > 0
        exact += walk["exact"]
        states.add(state)
        # the later rounds have known pixels to get wrong, under the mask, fp16 or not: with either ref (a loop frame runs both) in one
        # of the two images of the launch, and each image with one ref (the six pixels of a second row, where the flow's sign is the
        # image's, are known with one ref or the other)
        t = fs.loss_inputs(h, w)
        for flow in (t["flow"], t["flow16"]):
            later = np.stack([po.compute(flow[:2], t["mask"][:2], *fs.images(t, True, 1, (0, 1)), ref)["known"].reshape(2, -1)[:, stride:].sum(1)
                              for ref in po.REFS])
            assert (later.max(0) >= 5).all() and (later.max(1) >= 5).all(), (state, h, w, later.tolist())
        refs = [v["ref"] for v in fs.photometric_variants(h, w)]
        assert refs[0] != refs[3] and set(refs) == set(po.REFS)              # (the backward runs variants 0 and 3, the forward all four)
    assert states >= {"partial_second_round", "step_x_zero", "step_y_zero", "second_row"} and exact > 0
    assert backward or "three_rounds" in states
    # the frames of the family's own tests: the backward never loops there, the forward at 1080p alone
    for n, h, w in po.FRAMES:
        assert fs.photometric_walk(h, w, True)["rounds"] == 1 or (n, h, w) == po.LARGE
        assert (fs.photometric_walk(h, w, False)["rounds"] > 1) == ((n, h, w) == po.LARGE)


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
def test_the_smoothness_loop_frames_reach_their_states(backward):
    cap = G["smoothness"]["kMaxGradBlocks" if backward else "kMaxBlocks"]
    seen = set()
    for state, h, w in LOOPS["smoothness_bwd" if backward else "smoothness_fwd"]:
        walk = fs.smoothness_walk(h, w, backward)
        print(state, h, w, {k: v for k, v in walk.items()})
        assert walk["tiles"] > cap == walk["nblk"] and walk["rounds"] >= 2, (state, h, w)
        rag_row, rag_col = any(t[0] for t in walk["later"]), any(t[1] for t in walk["later"])
        assert rag_row and rag_col and any(t[0] and t[1] for t in walk["later"]), (state, h, w)      # a looping block meets the ragged corner
        assert any(t[3] for t in walk["later"]), (state, h, w)                                       # ... and re-stages a halo from inside the frame
        if state == "ragged_scalar":
            assert not walk["vec"] and walk["rounds"] == 2
        elif state == "ragged_vector":
            assert walk["vec"] and walk["rounds"] == 2
        else:
            assert state == "three_rounds" and walk["rounds"] == 3 and walk["tiles_x"] == 3 and any(t[2] for t in walk["later"])
        seen.add(state)
    assert seen == {"ragged_scalar", "ragged_vector", "three_rounds"}
    # the only looping frame of the family's own tests has full tiles alone
    n, h, w = so.FRAMES[-1]
    walk = fs.smoothness_walk(h, w, backward)
    assert walk["rounds"] == 2 + (not backward) * 6 and not any(t[0] or t[1] for t in walk["later"])
    assert all(fs.smoothness_walk(h, w, backward)["rounds"] == 1 for _, h, w in so.FRAMES[:-1])


def test_the_census_chunk_frames_reach_their_states():
    chunk = G["census"]["kChunk"]
    for state, h, w in LOOPS["census_finish"]:
        walk = fs.census_walk(h, w)
        print(state, h, w, walk)
        want = {"one_full_chunk": [(0, chunk)], "full_chunk_and_two": [(0, chunk), (chunk, 2)], "two_full_chunks": [(0, chunk), (chunk, chunk)],
                "three_chunks": [(0, chunk), (chunk, chunk), (2 * chunk, 1)]}[state]
        assert walk["chunks"] == want, (state, h, w)
        # what a wrong chunk base or a dropped chunk would change is there to be changed: in both images of the launch and at both
        # patches the records of every later chunk count known pixels, and the record before a chunk is not the chunk's last
        for patch in (3, 7):
            v = fs.census_chunk_variant(h, w, patch)
            a, mask, img, other = ls.photometric_operands(h, w, v, (0, 1))
            counts = fs.census_block_counts(cen.compute(a, mask, img, other, v["ref"], patch)["known"])
            for base, cnt in walk["chunks"][1:]:
                assert (counts[:, base:base + cnt] > 0).all(), (state, h, w, patch, counts[:, base:base + cnt].tolist())
                assert (counts[:, base - 1] != counts[:, base + cnt - 1]).all(), (state, h, w, patch)
    assert all(len(fs.census_walk(h, w)["chunks"]) == 1 and fs.census_walk(h, w)["nblk"] < chunk for _, h, w in cen.FRAMES)
    assert all(fs.census_walk(h, w)["nblk"] < chunk for h, w in fs.LOSS_TILE_FRAMES)


def test_the_epe_gradient_frame_reaches_the_second_round():
    (state, h, w), = LOOPS["epe_grad"]
    walk = fs.epe_grad_walk(h, w)
    assert state == "second_round" and walk["rounds"] == 2 and 0 < walk["last"] <= 8 and (h * w) % G["metrics"]["grad_pixels"] != 0
    assert fs.epe_grad_walk(1080, 1920)["rounds"] == 1                      # the largest frame of tests/test_gpu_flow_error.py


# ---- content ----------------------------------------------------------------------------------------------------------------------------
def _shares(h, w, images, patches=()):
    """Per image: the known share under the photometric oracle of both refs, the census oracle at `patches`, and the valid-term share
    of smoothness (x terms, order 1 and 2) under the mask -- each asserted to have both values."""
    t = fs.loss_inputs(h, w)
    sel = list(images)
    mask = t["mask"][sel]
    img, other = fs.images(t, True, 1, sel)
    out = []
    for ref in po.REFS:
        known = po.compute(t["flow"][sel], mask, img, other, ref)["known"]
        out.append(("photometric '%s'" % ref, known))
        for patch in patches:
            out.append(("census '%s' patch %d" % (ref, patch), cen.compute(t["flow"][sel], mask, img, other, ref, patch)["known"]))
    for order in (1, 2):
        if w > order:
            out.append(("smoothness order %d" % order, so.direction_terms(t["flow"][sel], mask, None, order, 10.0, 1e-3, 'x')["ok"]))
    low = 1.0
    for name, known in out:
        for i in range(len(sel)):
            if h * w >= 16:
                assert known[i].any() and not known[i].all(), "%d x %d image %d: %s has %s pixel" % (
                    h, w, sel[i], name, "no known" if not known[i].any() else "no unknown")
            if h * w >= 256:
                assert known[i].mean() >= 0.25, "%d x %d image %d: %s knows %.3f of the frame" % (h, w, sel[i], name, known[i].mean())
                low = min(low, float(known[i].mean()))
    return low


def test_every_tile_frame_has_known_and_unknown_pixels_under_each_oracle():
    low = min(_shares(h, w, ls.ALL, fs.CENSUS_PATCHES) for h, w in fs.LOSS_TILE_FRAMES)
    print("lowest known share on the tile frames: %.3f" % low)
    for h, w in fs.SMOOTHNESS_ONLY:
        t = fs.loss_inputs(h, w)
        assert t["flow"].shape == (4, 2, h, w) and t["mask"].shape == (4, h, w) and t["img"].shape == (4, 3, h, w)


def test_every_photometric_size_has_known_and_unknown_pixels():
    low = min(_shares(h, w, ls.ALL) for h, w in fs.photo_sizes())
    print("lowest known share on the photometric sizes: %.3f" % low)


@pytest.mark.parametrize("kernel", sorted(k for k in LOOPS if k != "epe_grad"))
def test_every_loop_frame_has_known_and_unknown_pixels(kernel):
    for state, h, w in LOOPS[kernel]:
        patches = (3,) if kernel == "census_finish" else ()
        low = _shares(h, w, (0, 1), patches)
        t = fs.loss_inputs(h, w)
        for key in ("flow", "mask", "img", "other"):                                     # the two images of a loop launch differ
            assert not np.array_equal(t[key][0], t[key][1]), (h, w, key)
        print("%s %s %d x %d: lowest known share %.3f" % (kernel, state, h, w, low))


def test_samples_leave_the_new_frames_over_every_border():
    new = fs.WIDE_LINE + [(h, w) for k, frames in LOOPS.items() if k != "epe_grad" for _, h, w in frames]
    for h, w in new:
        if min(h, w) < 8:
            continue                                                       # (content() makes no such promise on a short axis)
        sx, sy = fs.sample_positions(fs.loss_inputs(h, w)["flow"][:2])
        for side, where in dict(left=(sx < 0), right=(sx > w - 1), top=(sy < 0), bottom=(sy > h - 1)).items():
            assert where.any(), "%d x %d: no sample leaves across the %s border" % (h, w, side)
    assert sum(min(h, w) >= 8 for h, w in new) >= 20


def test_the_inputs_are_the_sweeps_content():
    for h, w in ((17, 36), (66, 133), (2, 35)):
        t, c = fs.loss_inputs(h, w), fs.content(h, w)
        assert np.array_equal(t["flow"], c["flow"]) and np.array_equal(t["mask"], c["m1"])
        assert np.array_equal(t["img"], c["src"][:, 0:3] / np.float32(255)) and np.array_equal(t["img_u8"], c["src"][:, 0:3].astype(np.uint8))
        assert np.array_equal(t["other"], c["src"][:, 3:6] / np.float32(255)) and np.array_equal(t["other_u8"], c["src"][:, 3:6].astype(np.uint8))
        assert t["flow16"].dtype == np.float16 and np.array_equal(t["flow16"], c["flow"].astype(np.float16))
        img, other = fs.images(t, False, 1)
        assert img.shape == (4, 1, h, w) and np.array_equal(img[:, 0], t["img"][:, 0]) and np.array_equal(other[:, 0], t["other"][:, 0])
        # a uint8 image reads as the fp32 one: s / 255 in float32 either way (photometric, smoothness)
        assert np.array_equal(po._as_image(t["img_u8"], 4), t["img"])


# ---- the comparison code ----------------------------------------------------------------------------------------------------------------
class Fakes:
    """The oracles in the bindings' place: the forward entry points are the oracles' own `fake_flow_*`; the gradients are the float64
    oracles rounded to float32.  `spoil(kind, array)` may change what a fake returns."""

    def __init__(self, monkeypatch, images):
        from oflibpytorch_amd import _census, _photometric, _smoothness
        self.up = tuple(fs.LOSS_UPSTREAM[i] for i in images)
        self.spoil = lambda kind, x: x
        monkeypatch.setattr(_photometric, "flow_photometric", self._forward(po.fake_flow_photometric))
        monkeypatch.setattr(_census, "flow_census", self._forward(cen.fake_flow_census))
        monkeypatch.setattr(_smoothness, "flow_smoothness", self._forward(so.fake_flow_smoothness))
        monkeypatch.setattr(_photometric, "flow_photometric_grad", self.photometric_grad)
        monkeypatch.setattr(_census, "flow_census_grad", self.census_grad)
        monkeypatch.setattr(_smoothness, "flow_smoothness_grad", self.smoothness_grad)

    def _forward(self, fake):
        def call(*args, **kw):
            rec, fmap = fake(*args, **kw)
            return (None if rec is None else torch.from_numpy(self.spoil("rec", rec.numpy().copy())),
                    None if fmap is None else torch.from_numpy(self.spoil("map", fmap.numpy().copy())))
        return call

    @staticmethod
    def _np(x):
        return None if x is None else x.numpy()

    def _grad(self, g):
        with np.errstate(over='ignore', invalid='ignore'):
            return torch.from_numpy(self.spoil("grad", np.asarray(g, np.float64).astype(np.float32)))

    def photometric_grad(self, vecs, mask, img, other, flow_sign, eps, scale):
        return self._grad(po.grad(vecs.numpy(), self._np(mask), img.numpy(), other.numpy(), 's' if flow_sign < 0 else 't', eps, self.up)[0])

    def census_grad(self, vecs, mask, img, other, flow_sign, patch, thresh, eps, q, scale):
        return self._grad(cen.grad(vecs.numpy(), self._np(mask), img.numpy(), other.numpy(), 's' if flow_sign < 0 else 't', patch, thresh,
                                   eps, q, self.up)[0])

    def smoothness_grad(self, vecs, mask, img, order, alpha, eps, scale):
        return self._grad(so.grad(vecs.numpy(), self._np(mask), self._np(img), order, alpha, eps, self.up)[0])


SMALL = [(2, 2), (5, 4), (17, 36), (17, 65), (34, 35), (17, 129)]


def test_the_comparisons_pass_on_the_oracles(oracle_native, monkeypatch):
    Fakes(monkeypatch, ls.ALL)
    tally = {}
    for h, w in SMALL:
        for v in fs.photometric_variants(h, w):
            ls.check_photometric(h, w, v, CPU, tally=tally)
        for v in fs.census_variants(h, w)[:6]:
            ls.check_census(h, w, v, CPU, tally=tally)
    for h, w in SMALL + fs.SMOOTHNESS_ONLY:
        for v in fs.smoothness_variants(h, w):
            ls.check_smoothness(h, w, v, CPU, tally=tally)
    assert tally["launches"] > 100 and tally["grad"] <= 1.0


def _steps_up(x, at):
    x[at] = np.nextafter(x[at], np.float32(np.inf))
    return x


def _moved(x, at):
    x[at] += np.abs(x[at[0]]).max() * np.float32(2.0 ** -12)
    return x


def _must_fail(call, text):
    with pytest.raises(AssertionError) as err:
        call()
    assert text in str(err.value), str(err.value)
    print(str(err.value)[:300])


def test_the_comparisons_fail_on_one_ulp_in_the_last_pixel_of_a_loop_frame(oracle_native, monkeypatch):
    """A forward loop frame of each kernel, two images.  The comparison passes on the oracle; it fails with the last pixel of the last
    image one float32 step up in the map; with the last gradient element moved by 2^-12 of the image's largest (the gradient's bar is
    2^-22 A + 1 ulp, at least 3 ulp and more where contributions cancel: a single step lies inside it); and with the record's sum short
    of one block."""
    fakes = Fakes(monkeypatch, (0, 1))
    cases = [(ls.check_photometric, LOOPS["photometric_fwd"][0][1:], dict(half=False, u8=True, ref='s', chan=1, masked=True), 1, "sum"),
             (ls.check_census, LOOPS["census_finish"][1][1:], dict(half=False, u8=True, ref='t', chan=1, masked=True, patch=3, q1=True), 1, ""),
             (ls.check_smoothness, LOOPS["smoothness_fwd"][0][1:], dict(order=1, kind=None, half=False, masked=False), 2, "sum_x")]
    for check, (h, w), v, sum_slot, sum_text in cases:
        run = lambda: check(h, w, v, CPU, images=(0, 1))
        fakes.spoil = lambda kind, x: x
        run()
        last = (1, h - 1, w - 1)
        fakes.spoil = lambda kind, x: _steps_up(x, last) if kind == "map" else x
        _must_fail(run, "first at %s" % (last,))
        fakes.spoil = lambda kind, x: _moved(x, (1, 1) + last[1:]) if kind == "grad" else x
        _must_fail(run, "the gradient")
        # one block record dropped from the sum of image 1: its share is sum / blocks, far over count * 2^-52 of the sum
        blocks = {ls.check_photometric: G["photometric"]["kMaxBlocks"], ls.check_census: fs.census_walk(h, w)["nblk"],
                  ls.check_smoothness: G["smoothness"]["kMaxBlocks"]}[check]

        def short(kind, x):
            if kind == "rec":
                x[1, sum_slot] -= x[1, sum_slot] / blocks
            return x
        fakes.spoil = short
        _must_fail(run, sum_text)
