"""GPU: engine.video_stabilize on the whole-pixel pans of tests/stab_ref.py, in grey and replicated to colour, with smooth None, 0
and 1 -- by the bits against the referee's path, maps and warp on the device's own pair models (which
tests/test_gpu_fit_motion.py holds to the referee's fit), and against frame 0 where the clip is locked to it."""
import numpy as np
import pytest

import fit_motion_ref as F
import stab_ref as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


def clip_for(colour):
    clip = S.pan_clip()
    return np.ascontiguousarray(np.stack([clip] * 3, axis=-1)) if colour else clip


@pytest.mark.parametrize("model", ["translation", "similarity", "affine"])
@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("smooth", [None, 0, 1])
def test_video_stabilize_equals_the_referee(eng, smooth, colour, model):
    import torch

    clip = clip_for(colour)
    border = "constant" if model == "affine" else "replicate"
    # a radius of 0: only matches that agree to the lattice point count, and whole-pixel pans of a texture are tracked exactly
    out, models, info, outside = eng.video_stabilize(torch.from_numpy(clip).cuda(), model=model, smooth=smooth, border=border, fill=77, thr=0.0,
                                                     hypotheses=64, seed=1)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == clip.shape
    assert tuple(models.shape) == (4, 6) and tuple(info.shape) == (4, 8) and tuple(outside.shape) == (5,) and outside.dtype == torch.int64
    out, models, info, outside = out.cpu().numpy(), models.cpu().numpy(), info.cpu().numpy(), outside.cpu().numpy()
    assert (info[:, 0] == F.FIT_OK).all()
    # the same pair models as the call on the grey clip
    m2, i2 = eng.video_camera_motion(torch.from_numpy(S.pan_clip()).cuda(), model=model, thr=0.0, hypotheses=64, seed=1)
    assert np.array_equal(m2.cpu().numpy().view(np.int64), models.view(np.int64)) and np.array_equal(i2.cpu().numpy(), info)
    # the engine's maps are the referee's, by the bits, and so is every frame
    if smooth != 0:
        assert np.array_equal(eng.stabilising_maps(models, info, smooth).view(np.int64), S.maps(models, info, smooth).view(np.int64))
    want, want_outside = S.stabilize(clip, models, info, smooth, border, 77)
    assert np.array_equal(out, want), f"{int((out != want).sum())} bytes differ"
    assert np.array_equal(outside, want_outside)
    if smooth == 0:
        assert np.array_equal(out, clip) and not outside.any()


@pytest.mark.parametrize("colour", [False, True])
def test_locked_to_frame_0_the_clip_equals_frame_0(eng, colour):
    import torch

    clip = clip_for(colour)
    out, models, info, outside = eng.video_stabilize(torch.from_numpy(clip).cuda(), model="similarity", smooth=None, border="constant", fill=200,
                                                     thr=0.0, hypotheses=64)
    out, models, info, outside = out.cpu().numpy(), models.cpu().numpy(), info.cpu().numpy(), outside.cpu().numpy()
    print("inliers per pair:", info[:, 5].tolist(), "of", info[:, 1].tolist())
    ys, xs = np.mgrid[0:S.CLIP_H, 0:S.CLIP_W]
    for b in range(4):
        dx, dy = S.OFFSETS[b][0] - S.OFFSETS[b + 1][0], S.OFFSETS[b][1] - S.OFFSETS[b + 1][1]
        assert models[b].tolist() == [1.0, 0.0, float(dx), 0.0, 1.0, float(dy)], (b, models[b])
    for f, (ox, oy) in enumerate(S.OFFSETS):
        inside = (xs - ox >= 0) & (xs - ox < S.CLIP_W) & (ys - oy >= 0) & (ys - oy < S.CLIP_H)
        assert outside[f] == S.pan_outside(ox, oy)
        assert np.array_equal(out[f][inside], clip[0][inside]) and (out[f][~inside] == 200).all(), f
