"""GPU tier of the loss sweep: flow_census_kernel / flow_census_grad_kernel<PATCH, HALF, U8> and flow_census_finish_kernel
(ofl_census.hip) on every tile frame of the sweep and in every state of the finish kernel's chunk loop, against tests/census_oracle.py
with the bars of tests/test_gpu_census.py (tests/loss_sweep.py).

n = 4, the four images of the frame's content.  A frame runs every (HALF, U8) at one patch each -- all three where the frame is no
larger than the widest halo -- forward and backward; the patch, the ref, the channels, the mask and q (1: the map bit for bit; the
default: within the pow's ulp) are spread by `frame_sweep.census_variants`, and tests/test_loss_sweep_host.py proves that each of the
twelve instantiations still meets every residue of the 64 x 16 tile.  The chunk frames (256, 258, 512 and 513 block records) run two
distinct images at patch 3 and 7, whose second must carry the bits of a launch of its own.  Every launch asserts the instantiation
the library reports."""
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


@pytest.mark.parametrize("half,u8", fs.TYPES, ids=TYPE_IDS)
def test_forward_and_backward_on_every_frame(half, u8, dev):
    tally, seen = {}, set()
    for h, w in fs.LOSS_TILE_FRAMES:
        for v in fs.census_variants(h, w):
            if (v["half"], v["u8"]) == (half, u8):
                ls.check_census(h, w, v, dev, name_of=_name, tally=tally)
                seen.add(v["patch"])
    assert seen == set(fs.CENSUS_PATCHES) and tally["launches"] >= len(fs.LOSS_TILE_FRAMES)
    print("%d launches, worst gradient element %.3f of its bound, worst map element at the default q %.2f ulp" % (
        tally["launches"], tally["grad"], tally["pow"]))


def test_a_frame_of_one_row_or_column_is_refused(dev):
    v = fs.census_variants(17, 36)[0]
    for h, w in fs.SMOOTHNESS_ONLY:
        with pytest.raises((RuntimeError, ValueError)):
            ls.run_census(h, w, v, dev, backward=False)


@pytest.mark.parametrize("state,h,w", LOOPS["census_finish"], ids=["%s-%dx%d" % f for f in LOOPS["census_finish"]])
def test_the_finish_kernels_chunks_in_every_state(state, h, w, dev):
    assert state == "one_full_chunk" or len(fs.census_walk(h, w)["chunks"]) >= 2
    for patch in (3, 7):
        v = fs.census_chunk_variant(h, w, patch)
        backward = (state, patch) == ("full_chunk_and_two", 7)               # the gradient too, on 258 tiles
        tally = {}
        both = ls.check_census(h, w, v, dev, images=(0, 1), backward=backward, name_of=_name, tally=tally)
        alone = ls.run_census(h, w, v, dev, images=(1,), backward=backward, name_of=_name)
        ls.same_run(both, alone, ls._what(h, w, v, (0, 1)) + ": image 1 of two and on its own", (slice(1, 2), slice(0, 1)))
        if backward:
            print("%s %d x %d: worst gradient element %.3f of its bound" % (state, h, w, tally["grad"]))


def test_two_launches_on_a_chunk_frame_give_the_same_bits(dev):
    state, h, w = LOOPS["census_finish"][1]
    v = dict(fs.census_chunk_variant(h, w, 7), q1=False)
    runs = [ls.run_census(h, w, v, dev, images=(0, 1), name_of=_name) for _ in range(2)]
    ls.same_run(runs[0], runs[1], "%d x %d, two launches" % (h, w))
