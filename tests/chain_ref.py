"""Referee of the displacement chain (ofx_displacement_chain, engine.displacement_chain, engine.chain_ring, engine.denoise_rings):
the definition in include/ofx.h ("displacement chain") restated in plain NumPy, every float32 operation spelled out and rounded
once, and what the engine builds on it.  Not a test module and not a conftest: tests import it.

tests/test_chain_ref.py pins the tap geometry and the blend against consistency_ref.consistency, which is pinned against
motion_ref.warp and, through it, against the oracle."""
import numpy as np

import temporal_ref

F32 = np.float32
FLT_MAX = F32(np.finfo(np.float32).max)
DEAD_BITS = 0x7FC00000
OK, LEAVES, UNDEFINED = 0, 2, 3
MAX_LINKS = 4


def step(acc, cls, link):
    """one link: (A_j, class) from A_{j-1} = acc [h, w, 2], the classes so far and D_j = link; parts: a dict of px, py, r_u and of
    which pixels read the link (live), leave at it (left), have no position (undefined) or fail step 5 (overflow)"""
    h, w, _ = acc.shape
    u, v = acc[..., 0], acc[..., 1]
    xs, ys = np.arange(w, dtype=F32)[None, :], np.arange(h, dtype=F32)[:, None]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        px = (xs + u).astype(F32)                                                  # 1.
        py = (ys + v).astype(F32)
        ok = (np.abs(px) <= F32(1e9)) & (np.abs(py) <= F32(1e9))                  # 2. (a NaN fails)
        gone = (px < F32(0)) | (px > F32(w - 1)) | (py < F32(0)) | (py > F32(h - 1))   # 3.
        alive = cls == OK
        live = alive & ok & ~gone
        sx, sy = np.where(live, px, F32(0)).astype(F32), np.where(live, py, F32(0)).astype(F32)
        x0, y0 = sx.astype(np.int64), sy.astype(np.int64)                         # 4. truncation; sx, sy >= 0
        fx, fy = (sx - x0.astype(F32)).astype(F32), (sy - y0.astype(F32)).astype(F32)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)

        def blend(plane):
            b00, b01, b10, b11 = plane[y0, x0], plane[y0, x1], plane[y1, x0], plane[y1, x1]
            a = (b00 + (fx * (b01 - b00).astype(F32)).astype(F32)).astype(F32)
            c = (b10 + (fx * (b11 - b10).astype(F32)).astype(F32)).astype(F32)
            return (a + (fy * (c - a).astype(F32)).astype(F32)).astype(F32)

        ru, rv = blend(link[..., 0]), blend(link[..., 1])
        su, sv = (u + ru).astype(F32), (v + rv).astype(F32)                       # 5.
        finite = (np.abs(su) <= FLT_MAX) & (np.abs(sv) <= FLT_MAX)
    new_cls = np.where(~alive, cls, np.where(~ok, UNDEFINED, np.where(gone, LEAVES, np.where(~finite, UNDEFINED, OK)))).astype(np.uint8)
    out = np.where((new_cls == OK)[..., None], np.stack([su, sv], -1), acc).astype(F32)
    return out, new_cls, {"px": px, "py": py, "ru": ru, "live": live, "left": alive & ok & gone, "undefined": alive & ~ok, "overflow": live & ~finite, "x0": x0, "y0": y0}


def chain(links, parts=False):
    """(dst float32 [h, w, 2], mask uint8 [h, w], stats int64 [4]) of the definition; with parts, also the list of step()'s dicts"""
    links = [np.asarray(l, F32) for l in links]
    assert 2 <= len(links) <= MAX_LINKS
    h, w, _ = links[0].shape
    assert all(l.shape == (h, w, 2) for l in links)
    acc, cls, seen = links[0].copy(), np.zeros((h, w), np.uint8), []
    for link in links[1:]:
        acc, cls, p = step(acc, cls, link)
        seen.append(p)
    dst = acc.view(np.uint32).copy()
    dst[cls != OK] = DEAD_BITS
    stats = np.array([w * h] + [int(np.count_nonzero(cls == c)) for c in (LEAVES, UNDEFINED, OK)], np.int64)
    out = (dst.view(F32), cls, stats)
    return out + (seen,) if parts else out


def chain_ring(ring, span):
    """engine.chain_ring: entry p is the chain of ring[p .. p + span - 1]"""
    ring = np.asarray(ring, F32)
    return np.stack([chain(list(ring[p:p + span]))[0] for p in range(len(ring) - span + 1)])


def denoise_rings(frames, fwd, bwd, weights, reach=1, centre_weight=256):
    """[(out, stats)] per frame of engine.denoise_rings: reach 1 is temporal_ref.denoise_rings; reach 2 adds frame f-2 through
    chain_ring(bwd, 2)[N-1-f] and frame f+2 through chain_ring(fwd, 2)[f], after the two near neighbours"""
    if reach == 1:
        return temporal_ref.denoise_rings(frames, fwd, bwd, weights, centre_weight)
    assert reach == 2
    frames = np.asarray(frames)
    N = len(frames)
    assert N >= 3
    fwd2, bwd2 = chain_ring(fwd, 2), chain_ring(bwd, 2)
    res = []
    for f in range(N):
        near = ([(frames[f - 1], bwd[N - 1 - f])] if f >= 1 else []) + ([(frames[f + 1], fwd[f])] if f + 1 < N else []) + \
               ([(frames[f - 2], bwd2[N - 1 - f])] if f >= 2 else []) + ([(frames[f + 2], fwd2[f])] if f + 2 < N else [])
        with np.errstate(invalid="ignore"):
            res.append(temporal_ref.temporal_filter(frames[f], [p for p, _ in near], [d for _, d in near], weights, centre_weight))
    return res
