"""NumPy referee of engine.video_camera_motion's fits and of engine.video_stabilize: klt_ref -> fit_motion_ref -> the camera
path, its moving average, the inverse maps -> warp_affine_ref.  Restated on its own: it shares no code with the engine."""
import numpy as np

import fit_motion_ref as F
import klt_ref as K
import warp_affine_ref as W

IDENT = np.array(F.IDENTITY, np.float64)


def camera_motion(frames, points, model, levels, prm, hypotheses, thr_q, refits, seed):
    """(models float64 [N - 1, 6], info int32 [N - 1, 8], positions float32 [N, n, 2], status int32 [n]) of one chain over the whole
    clip from caller's points: the referee's tracker on the referee's pyramids, then the fit per pair on the rows of the history"""
    h, w = frames[0].shape
    pyramids = [K.pyramid(f, levels) for f in frames]
    _, status, hist, _, _ = K.track_chain(pyramids, points, np.zeros(len(points), np.int32), 1, prm)
    pos = np.concatenate([np.asarray(points, np.float32)[None], hist])
    fits = [F.fit_motion(pos[b], pos[b + 1], (w, h), status, b + 1, model, hypotheses, thr_q, refits, seed) for b in range(len(frames) - 1)]
    return np.stack([f[0] for f in fits]), np.stack([f[1] for f in fits]), pos, status


def compose(m2, m1):
    a2, b2, x2, c2, d2, y2 = m2
    a1, b1, x1, c1, d1, y1 = m1
    return np.array([a2 * a1 + b2 * c1, a2 * b1 + b2 * d1, (a2 * x1 + b2 * y1) + x2, c2 * a1 + d2 * c1, c2 * b1 + d2 * d1, (c2 * x1 + d2 * y1) + y2])


def invert(m):
    a, b, x, c, d, y = m
    det = a * d - b * c
    assert det != 0 and np.isfinite(det)
    ia, ib, ic, id_ = d / det, -b / det, -c / det, a / det
    return np.array([ia, ib, -(ia * x + ib * y), ic, id_, -(ic * x + id_ * y)])


def maps(models, info, smooth):
    """W_f float64 [N, 6]: C_0 = I, C_f = M_f after C_{f-1} (M_f = I where the status is not OK); S_f the mean of C_g over the
    clipped window, summed in index order (None: S_f = I); W_f = C_f after the inverse of S_f"""
    models, info = np.asarray(models, np.float64), np.asarray(info)
    path = [IDENT.copy()]
    for f in range(len(models)):
        path.append(compose(models[f] if info[f][0] == F.FIT_OK else IDENT, path[-1]))
    if smooth is None:
        return np.stack(path)
    N, out = len(path), []
    for f in range(N):
        g0, g1 = max(f - smooth, 0), min(f + smooth, N - 1)
        s = np.zeros(6)
        for g in range(g0, g1 + 1):
            s = s + path[g]
        out.append(compose(path[f], invert(s / np.float64(g1 - g0 + 1))))
    return np.stack(out)


def stabilize(frames, models, info, smooth, border="replicate", fill=0):
    """(the stabilised clip, outside int64 [N]) from the pair models; frames [N, H, W] or [N, H, W, 3]"""
    frames = np.asarray(frames)
    if smooth == 0:
        return frames.copy(), np.zeros(len(frames), np.int64)
    w = maps(models, info, smooth)
    out = [W.warp_affine(frames[f], w[f], None, border, fill) for f in range(len(frames))]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int64)


# ---- the clip of the tests: whole-pixel pans of one texture ---------------------------------------------------------------------------
OFFSETS = [(0, 0), (4, 4), (1, 2), (3, 0), (-1, 3)]
CLIP_W, CLIP_H = 192, 128


def pan_clip():
    """five 192 x 128 crops of klt_ref.cosine_texture(224, 160) at OFFSETS: the content of frame 0 at (x, y) is at (x - ox, y - oy)"""
    big = K.cosine_texture(224, 160)
    return np.ascontiguousarray(np.stack([big[16 + oy:16 + oy + CLIP_H, 16 + ox:16 + ox + CLIP_W] for ox, oy in OFFSETS]))


def pan_outside(ox, oy):
    """the pixels of frame 0 that the crop at (ox, oy) does not hold"""
    return CLIP_W * CLIP_H - (CLIP_W - abs(ox)) * (CLIP_H - abs(oy))
