"""NumPy referee of "frame mosaic" (include/ofx.h; ofx_warp_mosaic) and of engine.stabilising_source_maps: restated from the
definition on top of warp_persp_ref.positions; it shares no code with the engine."""
import numpy as np

import homography_ref as R
import stab_ref as S
import warp_persp_ref as W
from fit_motion_ref import FIT_OK

MAX_SOURCES = 9
NONE = 255


def covers(src, m, size):
    """bool [h, w]: the output pixels whose position in `src` through m is defined and in range"""
    sh, sw = np.asarray(src).shape[:2]
    qx, qy, defined = W.positions(m, size[0], size[1])
    return defined & (qx >= 0) & (qx <= 32 * (sw - 1)) & (qy >= 0) & (qy <= 32 * (sh - 1))


def mosaic(srcs, models, size, border="replicate", fill=0):
    """(dst uint8 [h, w] or [h, w, 3], which uint8 [h, w], counts int64 [10]); srcs: 1 .. 9 uint8 images, models [S, 9], size (w, h)"""
    border = W.BORDERS.get(border, border)
    assert 1 <= len(srcs) <= MAX_SOURCES and len(models) == len(srcs)
    w, h = size
    # what a pixel shows when no source covers it: `fill`, or source 0 under replicate (`fill` where it is undefined)
    dst = W.warp_perspective(srcs[0], models[0], size, border, fill)[0].copy()
    if border == W.BORDER_CONSTANT:
        dst[...] = fill
    which = np.full((h, w), NONE, np.uint8)
    for k in range(len(srcs) - 1, -1, -1):                              # the smallest k that covers a pixel writes last
        c = covers(srcs[k], models[k], size)
        dst[c] = W.warp_perspective(srcs[k], models[k], size, W.BORDER_REPLICATE, fill)[0][c]
        which[c] = k
    counts = np.zeros(MAX_SOURCES + 1, np.int64)
    for k in range(len(srcs)):
        counts[k] = int((which == k).sum())
    counts[MAX_SOURCES] = int((which == NONE).sum())
    assert counts.sum() == w * h
    return dst, which, counts


def source_order(f, n, reach):
    """the source frames of output f: f, f - 1, f + 1, f - 2, f + 2, .. within the clip"""
    order = [f]
    for r in range(1, reach + 1):
        order += [f - r, f + r]
    return [g for g in order if 0 <= g < n]


def source_maps(models, info, smooth, reach):
    """(maps float64 [N, 1 + 2 reach, 9], frames int32 [N, 1 + 2 reach]) of engine.stabilising_source_maps"""
    models, info = np.asarray(models, np.float64), np.asarray(info)
    nine = models.ndim == 2 and models.shape[1] == 9
    if nine:
        ident = np.array(R.IDENTITY)
        path = [ident]
        for f in range(len(models)):
            path.append(R.normalize(R.compose(models[f] if info[f][0] == FIT_OK else ident, path[-1])))
        back = None if smooth is None else [R.invert(s) for s in R.smooth_path(np.stack(path), smooth)]
        entry = lambda g, f: path[g] if back is None else R.normalize(R.compose(path[g], back[f]))
    else:
        path = [S.IDENT.copy()]
        for f in range(len(models)):
            path.append(S.compose(models[f] if info[f][0] == FIT_OK else S.IDENT, path[-1]))
        back = None
        if smooth is not None:
            back = []
            for f in range(len(path)):
                g0, g1 = max(f - smooth, 0), min(f + smooth, len(path) - 1)
                s = np.zeros(6)
                for g in range(g0, g1 + 1):
                    s = s + path[g]
                back.append(S.invert(s / np.float64(g1 - g0 + 1)))
        entry = lambda g, f: R.from_affine(path[g] if back is None else S.compose(path[g], back[f]))
    n = len(path)
    maps = np.zeros((n, 1 + 2 * reach, 9), np.float64)
    frames = np.full((n, 1 + 2 * reach), -1, np.int32)
    for f in range(n):
        for k, g in enumerate(source_order(f, n, reach)):
            maps[f, k], frames[f, k] = entry(g, f), g
    return maps, frames


def filled(clip, maps, frames, border="replicate", fill=0):
    """[(dst, which, counts)] per frame: the mosaic of the clip's frames listed in row f through the maps of row f"""
    clip = np.asarray(clip)
    size = (clip.shape[2], clip.shape[1])
    out = []
    for f in range(len(clip)):
        n = int((frames[f] >= 0).sum())
        out.append(mosaic([clip[g] for g in frames[f, :n]], maps[f, :n], size, border, fill))
    return out
