"""GPU: engine.video_stabilize_filled -- every frame one mosaic item whose sources are the frame and its neighbours -- on the
whole-pixel pans of tests/stab_ref.py (by rectangle arithmetic, and against video_stabilize where nothing rounds) and on the 64 x 48
homography clip of tests/test_gpu_stabilize_homography.py, against tests/mosaic_ref.py of source_maps on the device's own pair
models, by the bits."""
import numpy as np
import pytest

import fit_motion_ref as F
import mosaic_ref as Z
import stab_ref as S
from test_gpu_stabilize_homography import MOTION, N, clip as homography_clip
from test_mosaic_ref import pan_covered

pytestmark = pytest.mark.gpu

PAN = dict(thr=0.0, hypotheses=64)            # tests/test_gpu_stabilize.py: the fitted models are the exact translations there


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


def colour_of(clip, colour):
    return np.ascontiguousarray(np.stack([clip] * 3, axis=-1)) if colour else clip


def filled(eng, clip, **kw):
    import torch

    res = eng.video_stabilize_filled(torch.from_numpy(clip).cuda(), **kw)
    assert len(res) == 5 and all(t.is_cuda for t in res)
    out, models, info, outside, borrowed = res
    assert out.dtype == torch.uint8 and tuple(out.shape) == clip.shape
    assert outside.dtype == torch.int64 and borrowed.dtype == torch.int64 and tuple(outside.shape) == tuple(borrowed.shape) == (len(clip),)
    return [t.cpu().numpy() for t in res]


def against_the_referee(eng, clip, res, smooth, reach, border, fill):
    out, models, info, outside, borrowed = res
    maps, frames = Z.source_maps(models, info, smooth, reach)
    got_maps, got_frames = eng.stabilising_source_maps(models, info, smooth, reach)
    assert got_maps.dtype == np.float64 and got_frames.dtype == np.int32 and np.array_equal(got_frames, frames)
    assert np.array_equal(got_maps.view(np.int64), maps.view(np.int64)), "stabilising_source_maps against the referee's, by the bits"
    for f, (dst, which, counts) in enumerate(Z.filled(clip, maps, frames, border, fill)):
        assert np.array_equal(out[f], dst), f"frame {f}: {int((out[f] != dst).sum())} bytes differ"
        assert outside[f] == counts[9] and borrowed[f] == counts[1:9].sum(), f


@pytest.mark.parametrize("colour", [False, True])
def test_locked_to_frame_0_the_pan_clip_is_frame_0_on_the_union_of_the_rectangles(eng, colour):
    import torch

    clip = colour_of(S.pan_clip(), colour)
    out, models, info, outside, borrowed = filled(eng, clip, model="similarity", smooth=None, reach=2, border="constant", fill=200, **PAN)
    assert (info[:, 0] == F.FIT_OK).all()
    for f in range(len(clip)):
        listed = [g for g in (f, f - 1, f + 1, f - 2, f + 2) if 0 <= g < len(clip)]
        covered, own = pan_covered(listed), pan_covered([f])
        assert np.array_equal(out[f][covered], clip[0][covered]) and (out[f][~covered] == 200).all(), f
        assert outside[f] == int((~covered).sum()) and borrowed[f] == int(covered.sum()) - int(own.sum()), f
    assert outside[4] == 7 and S.pan_outside(-1, 3) > 7
    # reach 0: video_stabilize's bytes and counts, since nothing rounds on whole pixels
    alone = filled(eng, clip, model="similarity", smooth=None, reach=0, border="constant", fill=200, **PAN)
    want = eng.video_stabilize(torch.from_numpy(clip).cuda(), model="similarity", smooth=None, border="constant", fill=200, **PAN)
    assert np.array_equal(alone[0], want[0].cpu().numpy()) and np.array_equal(alone[3], want[3].cpu().numpy()) and not alone[4].any()
    assert np.array_equal(alone[1].view(np.int64), want[1].cpu().numpy().view(np.int64))


@pytest.mark.parametrize("model", ["translation", "similarity", "affine"])
@pytest.mark.parametrize("colour", [False, True])
def test_the_smoothed_pan_clip_equals_the_referee(eng, colour, model):
    clip = colour_of(S.pan_clip(), colour)
    border = "constant" if model == "affine" else "replicate"
    res = filled(eng, clip, model=model, smooth=1, reach=2, border=border, fill=77, seed=1, **PAN)
    assert tuple(res[1].shape) == (4, 6) and (res[2][:, 0] == F.FIT_OK).all()
    against_the_referee(eng, clip, res, 1, 2, border, 77)
    assert res[4].any(), "pixels are borrowed from the neighbours"


@pytest.fixture(scope="module")
def alone(eng):
    """video_stabilize(model="homography") on the homography clip, per smooth: (clip, outside) as arrays"""
    import torch

    frames = torch.from_numpy(homography_clip()).cuda()
    res = {}
    for smooth in (None, 1):
        out, _, _, outside = eng.video_stabilize(frames, model="homography", smooth=smooth, border="constant", fill=77, **MOTION)
        res[smooth] = (out.cpu().numpy(), outside.cpu().numpy())
    return res


@pytest.mark.parametrize("smooth", [None, 1])
def test_the_homography_clip_equals_the_referee(eng, alone, smooth):
    clip = homography_clip()
    for reach in (1, 4):
        res = filled(eng, clip, model="homography", smooth=smooth, reach=reach, border="constant", fill=77, **MOTION)
        assert tuple(res[1].shape) == (N - 1, 9)
        against_the_referee(eng, clip, res, smooth, reach, "constant", 77)
        assert (res[3] <= alone[smooth][1]).all(), "a neighbour never uncovers a pixel"
    own = filled(eng, clip, model="homography", smooth=smooth, reach=0, border="constant", fill=77, **MOTION)
    assert np.array_equal(own[0], alone[smooth][0]) and np.array_equal(own[3], alone[smooth][1]) and not own[4].any()


@pytest.mark.parametrize("colour", [False, True])
def test_smooth_0_returns_the_clip(eng, colour):
    clip = colour_of(homography_clip(), colour)
    out, models, info, outside, borrowed = filled(eng, clip, model="homography", smooth=0, reach=2, **MOTION)
    assert np.array_equal(out, clip) and not outside.any() and not borrowed.any()
