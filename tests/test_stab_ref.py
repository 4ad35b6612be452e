"""CPU: the referees in a row -- klt_ref -> fit_motion_ref -> warp_affine_ref (tests/stab_ref.py) -- on whole-pixel pans of one
texture: every point stays alive, all three models come back as exact whole-pixel translations with every match an inlier at
radius 0, the clip locked to frame 0 equals frame 0 wherever its source is in range, and smooth 0 is the clip unchanged."""
import functools

import numpy as np
import pytest

import fit_motion_ref as F
import klt_ref as K
import stab_ref as S

PRM = K.Params(9, 20, 0, 0.0, 0)


@functools.lru_cache(maxsize=None)
def tracked():
    """the referee's chain over the clip, once: (positions [5, 40, 2], status [40])"""
    clip = S.pan_clip()
    pts = K.interior_points(S.CLIP_W, S.CLIP_H, 8, 5, 40)
    _, _, pos, status = S.camera_motion(clip, pts, "translation", 3, PRM, 1, 0, 0, 0)
    return pos, status


@functools.lru_cache(maxsize=None)
def fitted(model):
    pos, status = tracked()
    fits = [F.fit_motion(pos[b], pos[b + 1], (S.CLIP_W, S.CLIP_H), status, b + 1, model, 16, 0, 2, 0) for b in range(4)]
    return np.stack([f[0] for f in fits]), np.stack([f[1] for f in fits])


def test_every_point_stays_alive_and_moves_by_the_pan():
    pos, status = tracked()
    assert pos.shape == (5, 40, 2) and not status.any()
    for f, (ox, oy) in enumerate(S.OFFSETS):
        assert np.array_equal(pos[f], pos[0] - np.float32([ox, oy])), f


@pytest.mark.parametrize("model", ["translation", "similarity", "affine"])
def test_the_models_are_exact_whole_pixel_translations(model):
    models, info = fitted(model)
    for b in range(4):
        dx, dy = S.OFFSETS[b][0] - S.OFFSETS[b + 1][0], S.OFFSETS[b][1] - S.OFFSETS[b + 1][1]
        assert models[b].tolist() == [1.0, 0.0, float(dx), 0.0, 1.0, float(dy)], (b, models[b])
        assert info[b].tolist()[:2] == [F.FIT_OK, 40] and info[b][4] == 40 and info[b][5] == 40 and info[b][6] == 2


@pytest.mark.parametrize("model", ["translation", "similarity", "affine"])
@pytest.mark.parametrize("colour", [False, True])
def test_locked_to_frame_0_the_clip_equals_frame_0(model, colour):
    models, info = fitted(model)
    clip = S.pan_clip()
    if colour:
        clip = np.stack([clip, 255 - clip, clip // 2], axis=-1)
    w = S.maps(models, info, None)
    for f, (ox, oy) in enumerate(S.OFFSETS):
        assert w[f].tolist() == [1.0, 0.0, float(-ox), 0.0, 1.0, float(-oy)]
    for border in ("replicate", "constant"):
        out, outside = S.stabilize(clip, models, info, None, border, 77)
        assert out.shape == clip.shape and out.dtype == np.uint8
        ys, xs = np.mgrid[0:S.CLIP_H, 0:S.CLIP_W]
        for f, (ox, oy) in enumerate(S.OFFSETS):
            inside = (xs - ox >= 0) & (xs - ox < S.CLIP_W) & (ys - oy >= 0) & (ys - oy < S.CLIP_H)
            assert outside[f] == S.pan_outside(ox, oy) == int((~inside).sum())
            assert np.array_equal(out[f][inside], clip[0][inside]), (f, border)
            if border == "constant":
                assert (out[f][~inside] == 77).all()


def test_smooth_0_is_the_clip_unchanged_and_a_window_smooths():
    models, info = fitted("similarity")
    clip = S.pan_clip()
    out, outside = S.stabilize(clip, models, info, 0)
    assert np.array_equal(out, clip) and not outside.any()
    # smooth 1: the map of frame f is its position less the mean of its neighbours' -- whole thirds and halves of a pixel here
    w = S.maps(models, info, 1)
    path = -np.array(S.OFFSETS, np.float64)
    for f in range(5):
        g0, g1 = max(f - 1, 0), min(f + 1, 4)
        mean = path[g0:g1 + 1].sum(axis=0) / (g1 - g0 + 1)
        assert np.allclose(w[f], [1, 0, path[f][0] - mean[0], 0, 1, path[f][1] - mean[1]], rtol=0, atol=1e-12)
    # a pair whose fit failed counts as the identity
    bad = info.copy()
    bad[1, 0] = F.FIT_FEW
    assert S.maps(models, bad, None)[2].tolist() == S.maps(models, info, None)[1].tolist()
