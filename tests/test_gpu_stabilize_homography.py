"""GPU: the homography model of engine.video_camera_motion and engine.video_stabilize on a 64 x 48 clip of six frames, one texture
seen through known small homographies -- the pair models against the chain klt_ref -> homography_ref by the bits, the stabilised
frames against warp_persp_ref of the composed (and smoothed) path."""
import numpy as np
import pytest

import homography_ref as R
import klt_ref as K
import warp_persp_ref as W
from fit_motion_ref import FIT_OK

pytestmark = pytest.mark.gpu

CLIP_W, CLIP_H, N = 64, 48, 6
MOTION = dict(levels=2, window=7, cell=8, hypotheses=64, thr=0.5, refits=2, seed=3)


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


def views():
    """the inverse maps G_f of the frames: frame f shows the texture at G_f (x, y) -- a crop at (16, 16) that pans a little and tilts"""
    return [np.array([1.0 + 0.002 * f, 0.003 * f, 16.0 + 0.75 * f, -0.002 * f, 1.0 - 0.001 * f, 16.0 - 0.5 * f, 0.0002 * f, -0.00015 * f, 1.0]) for f in range(N)]


def clip():
    big = K.cosine_texture(CLIP_W + 32, CLIP_H + 32, fmax=0.45)
    frames = [W.warp_perspective(big, g, (CLIP_W, CLIP_H))[0] for g in views()]
    return np.ascontiguousarray(np.stack(frames))


def maps(models, info, smooth):
    """the referee's W_f [N, 9]: C_0 = I, C_f = normalize(M_f after C_{f-1}); S_f from smooth_path (None: I); W_f = normalize(C_f
    after the inverse of S_f)"""
    ident = np.array(R.IDENTITY)
    path = [ident]
    for f in range(len(models)):
        path.append(R.normalize(R.compose(models[f] if info[f][0] == FIT_OK else ident, path[-1])))
    path = np.stack(path)
    if smooth is None:
        return path
    s = R.smooth_path(path, smooth)
    return np.stack([R.normalize(R.compose(path[f], R.invert(s[f]))) for f in range(len(path))])


@pytest.fixture(scope="module")
def motion(eng):
    """(frames, the device's pair models and info as arrays), computed once"""
    import torch

    frames = clip()
    models, info = eng.video_camera_motion(torch.from_numpy(frames).cuda(), model="homography", **MOTION)
    assert models.is_cuda and tuple(models.shape) == (N - 1, 9) and models.dtype == torch.float64
    assert info.is_cuda and tuple(info.shape) == (N - 1, 8) and info.dtype == torch.int32
    return frames, models.cpu().numpy(), info.cpu().numpy()


def test_video_camera_motion_equals_the_referees_chain(eng, motion):
    frames, models, info = motion
    pyr = [eng.klt_pyramid(f, MOTION["levels"]).host() for f in frames]
    seeds, _ = eng.good_features(frames[0], MOTION["window"], MOTION["cell"])
    print("features:", len(seeds), "info:", info.tolist())
    assert len(seeds) >= 8
    _, status, hist, _, _ = K.track_chain(pyr, seeds, np.zeros(len(seeds), np.int32), 1, K.Params(MOTION["window"], 10, 1, 0.0, 0))
    pos = np.concatenate([np.asarray(seeds, np.float32)[None], hist])
    g = views()
    for b in range(N - 1):
        m, i, _ = R.fit_homography(pos[b], pos[b + 1], (CLIP_W, CLIP_H), status, b + 1, MOTION["hypotheses"], 16, MOTION["refits"], MOTION["seed"])
        assert info[b].tolist() == i.tolist(), f"pair {b + 1}: info {info[b].tolist()} vs {i.tolist()}"
        assert models[b].view(np.int64).tolist() == m.view(np.int64).tolist(), f"pair {b + 1}: {models[b].tolist()} vs {m.tolist()}"
        assert i[0] == FIT_OK and i[5] >= 6
        # the known motion: a point of frame b at x is at G_{b+1}^-1 G_b x in frame b + 1; to the half pixel a dozen tracks of a
        # 64 x 48 frame give at its corners
        truth = R.normalize(R.compose(R.invert(g[b + 1]), g[b]))
        corners = np.array([[0, 0], [CLIP_W - 1, 0], [0, CLIP_H - 1], [CLIP_W - 1, CLIP_H - 1]], np.float64)
        err = np.abs(R.apply(m, corners) - R.apply(truth, corners)).max()
        print(f"pair {b + 1}: corner error {err:.3f} px, {i[5]} inliers of {i[1]}")
        assert err <= 0.5


@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("smooth", [None, 1])
def test_video_stabilize_equals_the_referees_warp_of_the_path(eng, motion, smooth, colour):
    import torch

    frames, models, info = motion
    src = np.ascontiguousarray(np.stack([frames] * 3, axis=-1)) if colour else frames
    out, m2, i2, outside = eng.video_stabilize(torch.from_numpy(src).cuda(), model="homography", smooth=smooth, border="constant", fill=77, **MOTION)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == src.shape and tuple(outside.shape) == (N,)
    assert np.array_equal(m2.cpu().numpy().view(np.int64), models.view(np.int64)) and np.array_equal(i2.cpu().numpy(), info)
    w = maps(models, info, smooth)
    assert np.array_equal(eng.stabilising_maps(models, info, smooth).view(np.int64), w.view(np.int64))
    out, outside = out.cpu().numpy(), outside.cpu().numpy()
    for f in range(N):
        want, want_n = W.warp_perspective(src[f], w[f], None, "constant", 77)
        assert np.array_equal(out[f], want), f"frame {f}: {int((out[f] != want).sum())} bytes differ"
        assert outside[f] == want_n
    if smooth is None:
        assert np.array_equal(out[0], src[0]), "frame 0 is the anchor"
        # locked to frame 0, the inside of every frame shows what frame 0 shows there, up to resampling twice
        for f in range(1, N):
            inside = out[f] != 77
            diff = np.abs(out[f].astype(int) - src[0].astype(int))[inside]
            assert inside.mean() > 0.7 and np.mean(diff) < 6.0, (f, float(np.mean(diff)))


def test_smooth_0_returns_the_clip(eng, motion):
    import torch

    frames, models, info = motion
    out, m2, i2, outside = eng.video_stabilize(torch.from_numpy(frames).cuda(), model="homography", smooth=0, **MOTION)
    assert np.array_equal(out.cpu().numpy(), frames) and not outside.cpu().numpy().any()
    assert np.array_equal(m2.cpu().numpy().view(np.int64), models.view(np.int64))
