"""Referee of the stream pipeline's sampled output stage (ofx_sample_arrows / ofx_advect_points and the session calls on top of
them): the contract of include/ofx.h restated in plain NumPy with every float32 operation spelled out, plus the seeded
generator of synthetic flow pyramids the tests run it on.  Not a test module and not a conftest: tests import it.

The arrow field and the tracks are functions of the composed field C (main.cu:138-147) alone, so the referees take C as a
dense [h, w, 2] float32 array: oracle.compose_flow(...) of a flow pyramid in the GPU tests, compose() below (the same sum in
NumPy) or a hand-made array in the CPU tests."""
import numpy as np

F32 = np.float32


def compose(pyr, levels, level):
    """C at `level`: coarsest level first, u = (float)((double)u + 2^s * (double)flow_k[y >> s][x >> s].u), s = k - level."""
    h, w, _ = pyr[level].shape
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    acc = np.zeros((h, w, 2), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(levels - 1, level - 1, -1):
            s = k - level
            f = np.asarray(pyr[k], F32)[ys >> s, xs >> s]
            acc = (acc.astype(np.float64) + np.float64(1 << s) * f.astype(np.float64)).astype(F32)
    return acc


def arrow_grid(w, h, arrow_res):
    offset = w // arrow_res
    assert offset >= 1
    return offset, -(-h // offset), -(-w // offset)


def clamp_masks(C, arrow_res):
    """(u clamped, v clamped) at the grid points: which arrows the +-offset clamp changed."""
    h, w, _ = C.shape
    offset, _, _ = arrow_grid(w, h, arrow_res)
    g = C[::offset, ::offset]
    lim = F32(offset)
    with np.errstate(invalid="ignore"):
        return (g[..., 0] > lim) | (g[..., 0] < -lim), (g[..., 1] > lim) | (g[..., 1] < -lim)


def arrows(C, arrow_res):
    """[ny, nx, 4] int32 records (x0, y0, x1, y1) of the arrow field of C; an undrawn arrow has x1 = y1 = -1."""
    C = np.asarray(C, F32)
    h, w, _ = C.shape
    offset, ny, nx = arrow_grid(w, h, arrow_res)
    ii, jj = np.arange(0, h, offset), np.arange(0, w, offset)
    assert len(ii) == ny and len(jj) == nx
    g = C[ii][:, jj]
    u, v = g[..., 0], g[..., 1]
    fj, fi = jj.astype(F32)[None, :], ii.astype(F32)[:, None]
    lim = F32(offset)
    out = np.empty((ny, nx, 4), np.int32)
    with np.errstate(invalid="ignore"):
        # clamp: two comparisons, a NaN fails both and stays
        u = np.where(u > lim, lim, np.where(u < -lim, -lim, u)).astype(F32)
        v = np.where(v > lim, lim, np.where(v < -lim, -lim, v)).astype(F32)
        fx = (u + fj).astype(F32)                                        # one float32 add
        fy = (v + fi).astype(F32)
        nan = np.isnan(fx) | np.isnan(fy)
        x1 = np.trunc(np.where(nan, F32(0), fx)).astype(np.int32)       # (int): toward zero
        y1 = np.trunc(np.where(nan, F32(0), fy)).astype(np.int32)
    drawn = ~nan & (x1 >= 0) & (y1 >= 0)
    out[..., 0] = jj[None, :]
    out[..., 1] = ii[:, None]
    out[..., 2] = np.where(drawn, x1, -1)
    out[..., 3] = np.where(drawn, y1, -1)
    return out


def advect(C, points, status, pair):
    """One pair: (points', status') from float32 points [n, 2] of (x, y) and int32 status [n].  Vectorised over the points; every
    point sees the five steps of the contract in order."""
    C = np.asarray(C, F32)
    h, w, _ = C.shape
    pts = np.array(points, F32, copy=True)
    st = np.array(status, np.int32, copy=True)
    assert pts.ndim == 2 and pts.shape[1] == 2 and st.shape == (pts.shape[0],) and pair != 0
    x, y = pts[:, 0], pts[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        alive = st == 0                                                         # 1. frozen points do nothing
        inside = (x >= F32(0)) & (x < F32(w)) & (y >= F32(0)) & (y < F32(h))    # 2. NaN compares false
        st[alive & ~inside] = pair
        go = np.flatnonzero(alive & inside)
        xi, yi = x[go].astype(np.int32), y[go].astype(np.int32)                 # 3. (int): toward zero, here of values >= 0
        nx = (x[go] + C[yi, xi, 0]).astype(F32)                                 #    one float32 add each
        ny = (y[go] + C[yi, xi, 1]).astype(F32)
        fin = np.isfinite(nx) & np.isfinite(ny)
        st[go[~fin]] = pair                                                     # 4. not finite: lost, position kept
        pts[go[fin], 0] = nx[fin]                                               # 5.
        pts[go[fin], 1] = ny[fin]
    return pts, st


def track(fields, points, status=None, first_pair=1, n_slots=None):
    """Points through fields[0], fields[1], .. as pairs first_pair, first_pair + 1, ..  Returns (points, status, history) with
    history[q] the positions after pair first_pair + q -- or, with n_slots, the ring: slot (p - 1) mod n_slots."""
    pts = np.array(points, F32, copy=True)
    st = np.zeros(len(pts), np.int32) if status is None else np.array(status, np.int32, copy=True)
    hist = []
    for q, C in enumerate(fields):
        pts, st = advect(C, pts, st, first_pair + q)
        hist.append(pts.copy())
    if n_slots is not None:
        ring = [None] * n_slots
        for q, hp in enumerate(hist):
            ring[(first_pair + q - 1) % n_slots] = hp
        hist = ring
    return pts, st, hist


# ---- synthetic flow pyramids ----------------------------------------------------------------------------------------------------

def synth_pyramid(W, H, levels, level, seed, amp):
    """A flow pyramid of a W x H frame (levels `level` .. levels-1 filled, the others None) whose composed field at `level` has
    components of standard deviation ~amp: every level contributes the same variance.  Level `level` carries 2 % NaN, 1 % +Inf
    and 1 % -Inf components; the coarsest level one NaN and one Inf pixel (each poisons a whole block of the composition)."""
    rng = np.random.default_rng(seed)
    cnt = levels - level
    pyr = [None] * levels
    for k in range(level, levels):
        s = k - level
        f = rng.standard_normal((H >> k, W >> k, 2)) * (amp / ((1 << s) * np.sqrt(cnt)))
        pyr[k] = f.astype(F32)
    fine = pyr[level]
    r = rng.random(fine.shape)
    fine[r < 0.02] = np.nan
    fine[(r >= 0.02) & (r < 0.03)] = np.inf
    fine[(r >= 0.03) & (r < 0.04)] = -np.inf
    if cnt > 1:
        top = pyr[levels - 1]
        top[top.shape[0] // 2, top.shape[1] // 3, 0] = np.nan
        top[top.shape[0] // 3, top.shape[1] // 2, 1] = np.inf
    return pyr


def synth_points(w, h, n, seed):
    """n points of a w x h level: mostly uniform inside, the first few on and beyond the borders or not numbers."""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.random(n) * w, rng.random(n) * h], axis=1).astype(F32)
    pts = np.minimum(pts, np.array([np.nextafter(F32(w), F32(0)), np.nextafter(F32(h), F32(0))], F32))
    edge = np.array([[0, 0], [-0.0, 0.5], [w - 0.5, h - 0.5], [w, 1], [1, h], [-0.25, 3], [3, -1e-3], [np.nan, 2], [2, np.inf],
                     [-np.inf, 5]], F32)
    if n >= 4 * len(edge):
        pts[:len(edge)] = edge
    return pts


# (W, H, levels, level): the stateless calls' pyramids -- levels 2 to 5, level 0 and 1, odd coarsest widths (125 x 71, 41 x 25)
STATELESS_CASES = [(640, 480, 2, 0), (1000, 568, 4, 0), (1000, 568, 4, 1), (320, 240, 5, 0), (328, 200, 3, 1), (656, 400, 5, 1)]
ARROW_RES = [30, 7, "w"]
TRACK_PAIRS = 3     # pairs a synthetic track runs through
TRACK_AMP = 0.04    # composed flow's standard deviation per pair, as a fraction of the level's width


def arrow_case(case, arrow_res, seed=0):
    """(pyramid, arrow_res, w, h) of one stateless arrow case: the field's amplitude is the grid step, so about a third of the
    components clamp."""
    W, H, L, lv = case
    w, h = W >> lv, H >> lv
    res = w if arrow_res == "w" else arrow_res
    offset = w // res
    pyr = synth_pyramid(W, H, L, lv, 1000 + seed + 31 * STATELESS_CASES.index(case) + res, float(offset))
    # (a coarse grid may miss the sprinkled specials: three grid points get one each)
    pyr[lv][offset, offset, 0] = np.nan
    pyr[lv][offset, 2 * offset, 1] = np.inf
    pyr[lv][2 * offset, offset, 0] = -np.inf
    return pyr, res, w, h


def track_case(case, n_points, seed=0):
    """(pyramids of TRACK_PAIRS pairs, points, w, h) of one stateless track case."""
    W, H, L, lv = case
    w, h = W >> lv, H >> lv
    pyrs = [synth_pyramid(W, H, L, lv, 2000 + seed + 13 * q + L + lv, TRACK_AMP * w) for q in range(TRACK_PAIRS)]
    return pyrs, synth_points(w, h, n_points, 3000 + seed + n_points % 977), w, h
