"""GPU tier of the loss sweep: flow_smoothness_kernel<ORDER, IMG, BWD> (ofl_smoothness.hip) on every tile frame of the sweep and in
every state of its tile loop, against tests/smoothness_oracle.py with the bars of tests/test_gpu_smoothness.py (tests/loss_sweep.py;
DESIGN.md 4).

n = 4, the four images of the frame's content; the guidance image is the content's `img`.  A frame runs all six (ORDER, IMG)
instantiations, forward and backward -- the width decides between the 16-byte and the scalar form -- with fp16 storage and the mask
spread by `frame_sweep.smoothness_variants`; 1 x 5, 5 x 1 and 1 x 1 run here alone.  The loop frames (over 256 and 512 tiles forward,
1024 and 2048 backward, ragged in both axes, two and three tiles across) run two distinct images, whose second must carry the bits of a
launch of its own.  Every launch asserts the kernel the library reports."""
import pytest
import torch

import frame_sweep as fs
import loss_sweep as ls

pytestmark = pytest.mark.gpu
LOOPS = fs.loop_frames()
KIND_IDS = ["order%d-%s" % (o, i or "plain") for o, i in fs.SMOOTHNESS_KINDS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tier needs a HIP device"
    from oflibpytorch_amd import _native
    _native.load_library()
    return torch.device('cuda', 0)


def _name():
    from oflibpytorch_amd import _native
    return _native.last_kernel_name(demangle=False)


def _ids(frames):
    return ["%s-%dx%d" % f for f in frames]


@pytest.mark.parametrize("j", range(len(fs.SMOOTHNESS_KINDS)), ids=KIND_IDS)
def test_forward_and_backward_on_every_frame(j, dev):
    tally = {}
    frames = fs.LOSS_TILE_FRAMES + fs.SMOOTHNESS_ONLY
    for h, w in frames:
        ls.check_smoothness(h, w, fs.smoothness_variants(h, w)[j], dev, name_of=_name, tally=tally)
    assert tally["launches"] == len(frames)
    print("%s: %d frames, worst gradient element %.4f of its bound, worst map element %d ulp" % (KIND_IDS[j], len(frames), tally["grad"],
                                                                                                 tally.get("map", 0)))


def _pair_and_alone(h, w, v, dev, backward, tally):
    both = ls.check_smoothness(h, w, v, dev, images=(0, 1), backward=backward, name_of=_name, tally=tally)
    alone = ls.run_smoothness(h, w, v, dev, images=(1,), backward=backward, name_of=_name)
    ls.same_run(both, alone, ls._what(h, w, v, (0, 1)) + ": image 1 of two and on its own", (slice(1, 2), slice(0, 1)))


def _loop_variants(h, w):
    """Three of the frame's six: both orders, no image / fp32 / uint8 -- which three depends on the frame"""
    vs = fs.smoothness_variants(h, w)
    k = fs.frame_key(h, w) % 3
    return [vs[k], vs[3 + (k + 1) % 3], vs[(k + 2) % 3 + 3 * (k % 2)]]


@pytest.mark.parametrize("state,h,w", LOOPS["smoothness_fwd"], ids=_ids(LOOPS["smoothness_fwd"]))
def test_the_forward_tile_loop_in_every_state(state, h, w, dev):
    assert fs.smoothness_walk(h, w, False)["rounds"] >= 2
    for v in _loop_variants(h, w):
        _pair_and_alone(h, w, v, dev, False, None)


@pytest.mark.parametrize("state,h,w", LOOPS["smoothness_bwd"], ids=_ids(LOOPS["smoothness_bwd"]))
def test_the_backward_tile_loop_in_every_state(state, h, w, dev):
    assert fs.smoothness_walk(h, w, True)["rounds"] >= 2
    tally = {}
    for v in _loop_variants(h, w):
        _pair_and_alone(h, w, v, dev, True, tally)
    print("%s %d x %d: worst gradient element %.4f of its bound" % (state, h, w, tally["grad"]))


@pytest.mark.parametrize("kernel", ["smoothness_fwd", "smoothness_bwd"])
def test_two_launches_on_a_loop_frame_give_the_same_bits(kernel, dev):
    state, h, w = LOOPS[kernel][0]
    v = fs.smoothness_variants(h, w)[4]
    runs = [ls.run_smoothness(h, w, v, dev, images=(0, 1), name_of=_name) for _ in range(2)]
    ls.same_run(runs[0], runs[1], "%d x %d, two launches" % (h, w))
