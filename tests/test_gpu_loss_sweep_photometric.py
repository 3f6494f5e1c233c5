"""GPU tier of the loss sweep: flow_photometric_kernel<HALF, U8, BWD> (ofl_photometric.hip) on every frame of the sweep and in every
state of its grid-stride loop, against tests/photometric_oracle.py with the bars of tests/test_gpu_photometric.py (tests/loss_sweep.py;
DESIGN.md 4).

The kernel is one-dimensional over h w with 256 threads a block, so it runs on the tile frames (n = 4, the four images of the frame's
content) and on the sizes of the streaming sweep for E = 256.  A frame runs all four (HALF, U8) instantiations, forward and backward;
the ref, the channels and the mask are spread over the frames by `frame_sweep.photometric_variants`.  The loop frames
(`frame_sweep.loop_frames`: the smallest that reach each state of the walk, proved by tests/test_loss_sweep_host.py) run two distinct
images, whose second must carry the bits of a launch of its own.  Every launch asserts the instantiation the library reports."""
import pytest
import torch

import frame_sweep as fs
import loss_sweep as ls

pytestmark = pytest.mark.gpu
LOOPS = fs.loop_frames()
TYPE_IDS = ["%s-%s" % ("fp16" if hf else "fp32", "u8" if u8 else "f32") for hf, u8 in fs.TYPES]


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


@pytest.mark.parametrize("j", range(len(fs.TYPES)), ids=TYPE_IDS)
@pytest.mark.parametrize("frames", ["tiles", "sizes"])
def test_forward_and_backward_on_every_frame(frames, j, dev):
    tally = {}
    lst = fs.LOSS_TILE_FRAMES if frames == "tiles" else fs.photo_sizes()
    for h, w in lst:
        ls.check_photometric(h, w, fs.photometric_variants(h, w)[j], dev, name_of=_name, tally=tally)
    assert tally["launches"] == len(lst)
    print("%s %s: %d frames, worst gradient element %.3f of its bound" % (frames, TYPE_IDS[j], len(lst), tally["grad"]))


def test_a_frame_of_one_row_or_column_is_refused(dev):
    v = fs.photometric_variants(2, 5)[0]
    for h, w in fs.SMOOTHNESS_ONLY:
        with pytest.raises((RuntimeError, ValueError)):
            ls.run_photometric(h, w, v, dev, backward=False)


def _pair_and_alone(h, w, v, dev, backward, tally):
    """Images 0 and 1 of the frame against the oracle; image 1 of that launch carries the bits of a launch of image 1 alone."""
    both = ls.check_photometric(h, w, v, dev, images=(0, 1), backward=backward, name_of=_name, tally=tally)
    alone = ls.run_photometric(h, w, v, dev, images=(1,), backward=backward, name_of=_name)
    ls.same_run(both, alone, ls._what(h, w, v, (0, 1)) + ": image 1 of two and on its own", (slice(1, 2), slice(0, 1)))
    return both


@pytest.mark.parametrize("state,h,w", LOOPS["photometric_fwd"], ids=_ids(LOOPS["photometric_fwd"]))
def test_the_forward_loop_in_every_state(state, h, w, dev):
    assert fs.photometric_walk(h, w, False)["rounds"] >= 2
    for v in fs.photometric_variants(h, w):                                  # all four (HALF, U8)
        _pair_and_alone(h, w, v, dev, False, None)


@pytest.mark.parametrize("state,h,w", LOOPS["photometric_bwd"], ids=_ids(LOOPS["photometric_bwd"]))
def test_the_backward_loop_in_every_state(state, h, w, dev):
    assert fs.photometric_walk(h, w, True)["rounds"] >= 2
    tally = {}
    variants = fs.photometric_variants(h, w)
    for v in (variants[0], variants[3]):                                     # fp32 / fp32 and fp16 / uint8
        _pair_and_alone(h, w, v, dev, True, tally)
    print("%s %d x %d: worst gradient element %.3f of its bound" % (state, h, w, tally["grad"]))


@pytest.mark.parametrize("kernel", ["photometric_fwd", "photometric_bwd"])
def test_two_launches_on_a_loop_frame_give_the_same_bits(kernel, dev):
    state, h, w = LOOPS[kernel][0]
    v = fs.photometric_variants(h, w)[1]
    runs = [ls.run_photometric(h, w, v, dev, images=(0, 1), name_of=_name) for _ in range(2)]
    ls.same_run(runs[0], runs[1], "%d x %d, two launches" % (h, w))
