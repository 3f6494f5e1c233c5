"""GPU tier of the loss sweep for flow_ssim_kernel / flow_ssim_grad_kernel<WINDOW, HALF, U8> and flow_ssim_finish_kernel (ofl_ssim.hip)
on every tile frame of the sweep and in every state of the finish kernel's chunk loop, against tests/ssim_oracle.py with the bars of
tests/test_gpu_ssim.py (tests/loss_sweep_ssim.py).

n = 4, the four images of the frame's content.  Every (HALF, U8) at each window -- each of the twelve instantiations -- runs on every
frame of `frame_sweep.LOSS_TILE_FRAMES`, forward and backward; the ref, the channels and the mask are spread by
`frame_sweep.photometric_variants`.  The kernels keep the 64 x 16 tile and the 256-record chunk of the census kernels, so the chunk
frames are the census finish kernel's (256, 258, 512 and 513 block records): they run two distinct images at window 3 and 7, whose second
must carry the bits of a launch of its own.  Every launch asserts the instantiation the library reports."""
import pytest
import torch

import frame_sweep as fs
import loss_sweep as ls
import loss_sweep_ssim as lss

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


def test_the_kernels_keep_the_census_tile_and_chunk():
    assert lss.same_geometry_as_census() and lss.geometry() == dict(kTileW=64, kTileH=16, kChunk=256)


@pytest.mark.parametrize("window", lss.WINDOWS)
@pytest.mark.parametrize("half,u8", fs.TYPES, ids=TYPE_IDS)
def test_forward_and_backward_on_every_frame(half, u8, window, dev):
    tally = {}
    for h, w in fs.LOSS_TILE_FRAMES:
        v, = [v for v in lss.variants(h, w, window) if (v["half"], v["u8"]) == (half, u8)]
        lss.check(h, w, v, dev, name_of=_name, tally=tally)
    assert tally["launches"] == len(fs.LOSS_TILE_FRAMES)
    print("%d launches, worst gradient element %.3f of its bound" % (tally["launches"], tally["grad"]))


def test_a_frame_of_one_row_or_column_is_refused(dev):
    v = lss.variants(17, 36, 3)[0]
    for h, w in fs.SMOOTHNESS_ONLY:
        with pytest.raises((RuntimeError, ValueError)):
            lss.run(h, w, v, dev, backward=False)


@pytest.mark.parametrize("state,h,w", LOOPS["census_finish"], ids=["%s-%dx%d" % f for f in LOOPS["census_finish"]])
def test_the_finish_kernels_chunks_in_every_state(state, h, w, dev):
    assert lss.same_geometry_as_census()
    assert state == "one_full_chunk" or len(fs.census_walk(h, w)["chunks"]) >= 2
    for window in (3, 7):
        v = lss.chunk_variant(h, w, window)
        backward = (state, window) == ("full_chunk_and_two", 7)              # the gradient too, on 258 tiles
        tally = {}
        both = lss.check(h, w, v, dev, images=(0, 1), backward=backward, name_of=_name, tally=tally)
        alone = lss.run(h, w, v, dev, images=(1,), backward=backward, name_of=_name)
        ls.same_run(both, alone, ls._what(h, w, v, (0, 1)) + ": image 1 of two and on its own", (slice(1, 2), slice(0, 1)))
        if backward:
            print("%s %d x %d: worst gradient element %.3f of its bound" % (state, h, w, tally["grad"]))


def test_two_launches_on_a_chunk_frame_give_the_same_bits(dev):
    state, h, w = LOOPS["census_finish"][1]
    v = lss.chunk_variant(h, w, 7)
    runs = [lss.run(h, w, v, dev, images=(0, 1), name_of=_name) for _ in range(2)]
    ls.same_run(runs[0], runs[1], "%d x %d, two launches" % (h, w))
