"""Referee of colour frame interpolation (ofx_interpolate_frames_3ch, ofx_interpolate_frames_3ch_batch,
engine.interpolate_frames_colour, engine.video_interpolate_colour, engine.video_interpolate_colour_dense): the definition "colour
frame interpolation" in include/ofx.h says that channel c of the result IS "frame interpolation" of the planes a[..., c] and
b[..., c], so the referee is tests/interp_ref.py run per channel -- plus the seeded inputs the CPU and the GPU tests share.  Not a
test module and not a conftest: tests import it."""
import functools

import numpy as np

import interp_ref as R

SEEDS = (0, 11, 23)            # planes3: the channels' seeds are these plus 100 * seed
Q_SEEDS = (41, 7, 3)           # colour_quality_clip: the channels' textures


@functools.lru_cache(maxsize=None)
def planes3(w, h, seed=0):
    """(a, b) uint8 [h, w, 3]: the channels are independent interp_ref.planes of different seeds"""
    ch = [R.planes(w, h, 100 * seed + s) for s in SEEDS]
    out = tuple(np.ascontiguousarray(np.stack([c[i] for c in ch], axis=2)) for i in (0, 1))
    for p in out:
        p.setflags(write=False)
    return out


def interpolate3(a, b, dab, dba, t):
    """(out uint8 [h, w, 3], stats int64 [4], cls uint8 [h, w]) of the definition at one time t: interp_ref.interpolate per channel;
    the geometry does not look at the planes, so the three stats and class maps agree"""
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    assert a.ndim == 3 and a.shape[2] == 3 and b.shape == a.shape
    res = [R.interpolate(a[..., c], b[..., c], dab, dba, t) for c in range(3)]
    for r in res[1:]:
        assert np.array_equal(r[1], res[0][1]) and np.array_equal(r[2], res[0][2])
    return np.ascontiguousarray(np.stack([r[0] for r in res], axis=2)), res[0][1], res[0][2]


def interpolate3_times(a, b, dab, dba, times):
    """(frames uint8 [T, h, w, 3], stats int64 [T, 4]) of the definition at every time"""
    res = [interpolate3(a, b, dab, dba, t) for t in times]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


@functools.lru_cache(maxsize=None)
def reference3(kind, w, h, ts, seed=0):
    """(frames [T, h, w, 3], stats [T, 4]) of planes3(w, h, seed), interp_ref.field_case(kind, w, h, seed) at TIME_SETS[ts];
    computed once, not to be written to"""
    a, b = planes3(w, h, seed)
    dab, dba = R.field_case(kind, w, h, seed)
    out = interpolate3_times(a, b, dab, dba, R.TIME_SETS[ts])
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def colour_quality_clip(step):
    """nine colour frames [Q_H, Q_W, 3] of three moving textures (one per channel, all with the same motion): frames 0, 4, 8 are
    the clip, the others the truth at t = 1/4, 1/2, 3/4"""
    from cuda_optical_flow_2_amd import synth

    frames = []
    for i in range(9):
        f = np.ascontiguousarray(np.stack([synth.smooth_pair(R.Q_W, R.Q_H, step[0] * i, step[1] * i, seed=s)[1] for s in Q_SEEDS], axis=2))
        f.setflags(write=False)
        frames.append(f)
    return tuple(frames)


def grey(img):
    """(c0 + c1 + c2) // 3: OFX_FRONTEND_GREY's value"""
    img = np.asarray(img)
    return ((img[..., 0].astype(np.int64) + img[..., 1] + img[..., 2]) // 3).astype(np.uint8)
