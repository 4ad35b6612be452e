"""CPU: the referee of the frame mosaic (tests/mosaic_ref.py) on the inputs of tests/mosaic_cases.py -- the conditions that keep
tests/test_gpu_mosaic.py from passing vacuously (every source index and 255 occur, a wave that source 0 resolves alone and one that
needs three, undefined pixels that a later source covers, uncovered pixels of both kinds) -- and the consequences the definition
states; stabilising_source_maps' referee against the stabiliser's maps, and the filled pan clip by rectangle arithmetic."""
import numpy as np
import pytest

import homography_ref as R
import mosaic_cases as M
import mosaic_ref as Z
import stab_ref as S
import warp_persp_ref as W
from fit_motion_ref import FIT_OK

BIG = [(33, 17), (67, 45), (262, 74)]


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("S_", M.LADDER_S)
@pytest.mark.parametrize("size", BIG)
def test_the_ladder_reaches_every_source_and_none(size, S_, channels):
    name, srcs, models, size = M.ladder(size[0], size[1], S_, channels)
    assert len({s.shape for s in srcs}) == min(S_, 3), "sources of different sizes"
    for border in ("replicate", "constant"):
        dst, which, counts = Z.mosaic(srcs, models, size, border, 99)
        assert sorted(set(which.reshape(-1).tolist())) == list(range(S_)) + [255], name
        assert all(counts[k] > 0 for k in range(S_)) and not counts[S_:9].any() and counts[9] > 0 and counts.sum() == size[0] * size[1]
        if border == "constant":
            assert (dst[which == 255] == 99).all()
        else:
            # the uncovered pixels show source 0 at its clamped position: defined there, since its model is affine
            alone = W.warp_perspective(srcs[0], models[0], size, "replicate", 99)[0]
            assert W.positions(models[0], *size)[2].all() and np.array_equal(dst[which == 255], alone[which == 255])
    # the priority decides where two sources share a column
    shared = sum(int((Z.covers(srcs[a], models[a], size) & Z.covers(srcs[b], models[b], size)).sum()) for a in range(S_) for b in range(a))
    assert shared > 0 or S_ == 1


def test_the_shake_has_a_wave_of_one_source_and_a_wave_of_three():
    name, srcs, models, size = M.shake(262, 74, 1)
    dst, which, counts = Z.mosaic(srcs, models, size, "replicate", 0)
    per_wave = M.waves(which)
    assert sum(len(v) for v in per_wave) == 262 * 74
    assert any(len(v) == M.WAVE_PX and (v == 0).all() for v in per_wave), "a wave that leaves the loop after source 0"
    assert any(len(set(v.tolist())) >= 3 for v in per_wave), "a wave that goes on to a third source"
    assert counts[0] > 0.9 * which.size and (counts[1:5] > 0).all()
    # an aligned 256-pixel run of a row that source 0 covers, and a run with three values
    assert (which[10, :256] == 0).all()
    assert max(len(set(which[y, x0:x0 + 256].tolist())) for y in range(74) for x0 in (0, 6)) >= 3


@pytest.mark.parametrize("shape", M.SHAPES[3:])
def test_the_hard_models_leave_pixels_to_the_second_source_and_to_nobody(shape):
    """Four of the hard models leave undefined pixels, which the covering second source takes; "far" and "limits" are defined at every
    pixel of these shapes and out of range, so there source 1 takes pixels that source 0 merely does not cover.  With the second
    source over the left half only, pixels stay uncovered where source 0 is undefined and where it is defined."""
    w, h, sw, sh = shape
    seen_undefined_uncovered = seen_defined_uncovered = False
    for name, srcs, models, size in M.hard_pairs(w, h, sw, sh, 1):
        defined = W.positions(models[0], w, h)[2]
        dst, which, counts = Z.mosaic(srcs, models, size, "replicate", 41)
        assert (which == 1).any(), f"{name}: source 0 leaves pixels that source 1 covers"
        if name.split(",")[0] in ("horizon inside", "W = 0 at pixels", "W < 0 everywhere", "tiny W"):
            assert not defined.all(), name
        else:
            assert defined.all(), f"{name}: defined at every pixel, and out of range"          # ("far", "limits")
        if name.endswith("full"):
            assert defined.all() or ((which == 1) & ~defined).any(), f"{name}: source 0 undefined and source 1 covers"
            assert counts[9] == 0 and counts[0] + counts[1] == w * h
        else:
            assert counts[9] > 0
            none = which == 255
            seen_undefined_uncovered |= bool((none & ~defined).any())
            seen_defined_uncovered |= bool((none & defined).any())
            assert (dst[none & ~defined] == 41).all()
            alone = W.warp_perspective(srcs[0], models[0], size, "replicate", 41)[0]
            assert np.array_equal(dst[none], alone[none])
    assert seen_undefined_uncovered and seen_defined_uncovered


@pytest.mark.parametrize("channels", [1, 3])
def test_one_source_is_the_perspective_warp(channels):
    for w, h, sw, sh in M.SHAPES:
        src = M.image(sw, sh, channels)
        for name, m in M.models_for(w, h, sw, sh):
            for border in ("replicate", "constant"):
                dst, which, counts = Z.mosaic([src], [m], (w, h), border, 17)
                want, outside = W.warp_perspective(src, m, (w, h), border, 17)
                assert np.array_equal(dst, want) and counts[9] == outside and counts[0] == w * h - outside, (name, border)
                assert set(which.reshape(-1).tolist()) <= {0, 255}


def test_appending_a_source_leaves_covered_pixels_alone():
    for case in (M.ladder(67, 45, 9, 3), M.shake(67, 45, 1)):
        name, srcs, models, size = case
        for border in ("replicate", "constant"):
            prev = None
            for n in range(1, len(srcs) + 1):
                dst, which, counts = Z.mosaic(srcs[:n], models[:n], size, border, 5)
                if prev is not None:
                    kept = prev[1] != 255
                    assert np.array_equal(dst[kept], prev[0][kept]) and np.array_equal(which[kept], prev[1][kept]), (name, n)
                    assert set(which[~kept].tolist()) <= {n - 1, 255}
                prev = (dst, which)


def test_one_plane_given_twice_is_taken_once():
    src = M.image(40, 30, 1)
    m = (1.0, 0.0, 3.25, 0.0, 1.0, -2.5, 0.0, 0.0, 1.0)
    dst, which, counts = Z.mosaic([src, src], [m, m], (40, 30), "constant", 0)
    assert counts[1] == 0 and counts[0] > 0 and counts[9] > 0


def pan_models():
    """the exact pair models of stab_ref.pan_clip(): whole-pixel translations"""
    o = S.OFFSETS
    return np.array([[1.0, 0.0, float(o[b][0] - o[b + 1][0]), 0.0, 1.0, float(o[b][1] - o[b + 1][1])] for b in range(len(o) - 1)])


def pan_covered(frames):
    """bool [H, W]: the pixels of frame 0's plane inside the union of the listed frames' rectangles, by rectangle arithmetic"""
    ys, xs = np.mgrid[0:S.CLIP_H, 0:S.CLIP_W]
    c = np.zeros((S.CLIP_H, S.CLIP_W), bool)
    for g in frames:
        ox, oy = S.OFFSETS[g]
        c |= (xs - ox >= 0) & (xs - ox < S.CLIP_W) & (ys - oy >= 0) & (ys - oy < S.CLIP_H)
    return c


def info_ok(n):
    info = np.zeros((n, 8), np.int32)
    info[:, 0] = FIT_OK
    return info


def test_source_maps_own_entries_are_the_stabilisers_maps():
    models6 = pan_models() + np.array([0.001, -0.002, 0.3, 0.002, 0.0015, -0.2]) * np.arange(1, 5)[:, None]
    info = info_ok(4)
    info[2, 0] = FIT_OK + 1                                            # a pair that failed: the identity
    for smooth in (None, 1, 2):
        for reach in (0, 2, 4):
            maps, frames = Z.source_maps(models6, info, smooth, reach)
            assert maps.shape == (5, 1 + 2 * reach, 9) and frames.shape == (5, 1 + 2 * reach) and frames.dtype == np.int32
            own = np.stack([R.from_affine(m) for m in S.maps(models6, info, smooth)])
            assert np.array_equal(maps[:, 0].view(np.int64), own.view(np.int64))
            for f in range(5):
                want = [g for g in [f] + [g for r in range(1, reach + 1) for g in (f - r, f + r)] if 0 <= g < 5]
                assert frames[f].tolist() == want + [-1] * (1 + 2 * reach - len(want))
                assert not maps[f, len(want):].any()
    from test_gpu_stabilize_homography import maps as homography_maps, views

    g = views()
    models9 = np.stack([R.normalize(R.compose(R.invert(g[b + 1]), g[b])) for b in range(len(g) - 1)])
    info = info_ok(len(models9))
    for smooth in (None, 1):
        maps, frames = Z.source_maps(models9, info, smooth, 1)
        assert np.array_equal(maps[:, 0].view(np.int64), homography_maps(models9, info, smooth).view(np.int64))
        assert frames[0].tolist() == [0, 1, -1] and frames[3].tolist() == [3, 2, 4]


def test_the_filled_pan_clip_equals_frame_0_on_the_union_of_the_rectangles():
    clip = S.pan_clip()
    maps, frames = Z.source_maps(pan_models(), info_ok(4), None, 2)
    res = Z.filled(clip, maps, frames, "constant", 200)
    for f, (dst, which, counts) in enumerate(res):
        listed = [g for g in frames[f] if g >= 0]
        covered = pan_covered(listed)
        assert np.array_equal(which != 255, covered), f
        assert np.array_equal(dst[covered], clip[0][covered]) and (dst[~covered] == 200).all(), f
        assert counts[9] == int((~covered).sum()) and counts[0] == S.CLIP_W * S.CLIP_H - S.pan_outside(*S.OFFSETS[f])
        assert counts[1:9].sum() == int(covered.sum()) - int(pan_covered([f]).sum())
    assert frames[4].tolist() == [4, 3, 2, -1, -1]
    assert res[4][2][9] == 7 and S.pan_outside(-1, 3) == 192 * 128 - 191 * 125
