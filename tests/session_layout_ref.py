"""The arithmetic of ofx_session_create as it stood before csrc/session_plan.h held it: a transcription, in Python, of lines 65-253 of
csrc/session.cpp in commit 4fac30a ("Fused iteration launch: keep the warp's tap loads in flight over joins") -- the levels'
geometry, the flags, the offset vectors (off_plane, off_flow, off_flow2, off_flow_alt, flow_stride, off_patch, off_pscr, pscr_frame),
the pointers made from them forty lines further down, and the total -- and of the rule of its lines 34-35 (a single-level session
with iterations copies its frames).  Transcribed from that function, statement by statement and with its names, NOT from the new
header: tests/test_session_plan.py compares the header's plans with it, tests/test_gpu_session_layout.py the pointers of real
sessions.  The checks of ofx_params of its lines 37-62 are not here; the three error exits of the layout are (LayoutError)."""

K_MAX_BATCH = 16            # OFX_STREAM_MAX_BATCH
K_SETS = 3 * K_MAX_BATCH + 2
K_UV_SLOTS = 2 * K_MAX_BATCH
K_ALIGN = 256
MAX_LEVELS = 12             # OFX_MAX_LEVELS
MODE_COMPAT_CPU, MODE_LK_FLOAT, MODE_LK_FLOAT_FAST = 0, 1, 2
ITER_PAIRS_DEFAULT = 1      # OFX_ITER_PAIRS_DEFAULT

PARAMS = dict(width=0, height=0, levels=1, window=9, mode=MODE_LK_FLOAT, device=0, sharded=0, own_y0=(), own_y1=(), buf_y0=(), buf_y1=(),
              comp_y0=(), comp_y1=(), iters=0, local_corner=0, patch_size=0, stream_batch=0, borrow_frames=0, min_det=0.0, stream_two_stage=0,
              frames_partial=0, deep_fetch=0)
# the environment as the function read it: None = the variable is not set, else its atoi
ENV = dict(OFX_ITER_FUSED=None, OFX_ITER_PAIRS=None, OFX_ITER_DMA=None, OFX_PAIR_PACK=None, OFX_PAIR_WAVES=None, OFX_DEBUG_CORNER_EXTENT=None)


class LayoutError(Exception):
    """One of the function's three `ofx_set_error(...); delete s; return OFX_E_INVALID;` exits."""


def align_up(v, a):
    return (v + a - 1) // a * a


def layout(params, env=None):
    """params: the fields of ofx_params that differ from PARAMS; env: the variables that are set.  Returns a dict: the levels' fields as
    lists, the flags, `at` = {(name, i, j, k): byte offset} for every non-null pointer of the session, and `total`."""
    p = dict(PARAMS, **params)
    e = dict(ENV, **(env or {}))
    rows = {n: list(p[n]) + [0] * (MAX_LEVELS - len(p[n])) for n in ("own_y0", "own_y1", "buf_y0", "buf_y1", "comp_y0", "comp_y1")}
    # :34-35
    if p["levels"] == 1 and p["iters"] > 1 and p["borrow_frames"]:
        p["borrow_frames"] = p["stream_two_stage"] = 0
    L = p["levels"]
    s = {n: [0] * L for n in "w h pitch own0 own1 buf0 buf1 cmp0 cmp1 fl0 fl1 pw ph ppitch".split()}
    # :70-81
    B = p["stream_batch"] if p["stream_batch"] >= 2 else 1                       # stream_batch_of (session.h)
    n_sets = (2 if p["stream_two_stage"] else 3) * B + 2                         # stream_sets (session.h)
    total = 0
    n_iter_sets = 3 * B if p["iters"] > 1 else 0
    off_plane = [[] for _ in range(K_SETS + 2 + 3 * K_MAX_BATCH)]
    off_flow, off_flow2, off_flow_alt, flow_stride = [], [], [], []
    want_pairs = (p["iters"] >= 3 and not p["sharded"] and p["mode"] in (MODE_LK_FLOAT, MODE_LK_FLOAT_FAST)
                  and (p["window"] >> 1) >= 1 and (p["window"] >> 1) <= 4 and p["width"] * p["height"] < 16 * 1000 * 1000
                  and (e["OFX_ITER_DMA"] is None or e["OFX_ITER_DMA"] <= 0)
                  and (e["OFX_ITER_PAIRS"] != 0 if e["OFX_ITER_PAIRS"] is not None else ITER_PAIRS_DEFAULT != 0))
    plane_bytes_of = []
    # :82-134
    for k in range(L):
        s["w"][k] = p["width"] >> k
        s["h"][k] = p["height"] >> k
        s["pitch"][k] = align_up(s["w"][k], 64)
        if p["sharded"]:
            s["own0"][k] = rows["own_y0"][k]
            s["own1"][k] = rows["own_y1"][k]
            s["buf0"][k] = rows["buf_y0"][k]
            s["buf1"][k] = rows["buf_y1"][k]
            has_comp = rows["comp_y1"][k] > 0
            s["cmp0"][k] = rows["comp_y0"][k] if has_comp else s["own0"][k]
            s["cmp1"][k] = rows["comp_y1"][k] if has_comp else s["own1"][k]
            ok = (0 <= s["buf0"][k] and s["buf0"][k] <= s["own0"][k] and s["own0"][k] <= s["own1"][k]
                  and s["own1"][k] <= s["buf1"][k] and s["buf1"][k] <= s["h"][k] and s["buf0"][k] < s["buf1"][k]
                  and s["buf0"][k] <= s["cmp0"][k] and s["cmp0"][k] <= s["own0"][k] and s["own1"][k] <= s["cmp1"][k]
                  and s["cmp1"][k] <= s["buf1"][k])
            if not ok:
                raise LayoutError("ofx_session_create: level %d shard rows own [%d,%d) buf [%d,%d) invalid for height %d"
                                  % (k, s["own0"][k], s["own1"][k], s["buf0"][k], s["buf1"][k], s["h"][k]))
        else:
            s["own0"][k] = s["buf0"][k] = s["cmp0"][k] = 0
            s["own1"][k] = s["buf1"][k] = s["cmp1"][k] = s["h"][k]
        s["fl0"][k] = s["own0"][k]
        s["fl1"][k] = s["own1"][k]
        if p["sharded"] and p["iters"] > 1:
            reach = (p["window"] >> 1) + 1
            ext = reach * (p["iters"] - 1)
            s["fl0"][k] = s["own0"][k] - ext if s["own0"][k] - ext > 0 else 0
            s["fl1"][k] = s["own1"][k] + ext if s["own1"][k] + ext < s["h"][k] else s["h"][k]
            lo = s["fl0"][k] - reach if s["fl0"][k] - reach > 0 else 0
            hi = s["fl1"][k] + reach if s["fl1"][k] + reach < s["h"][k] else s["h"][k]
            if lo < s["buf0"][k] or hi > s["buf1"][k]:
                raise LayoutError("ofx_session_create: level %d: %d iterations need rows [%d,%d) in the buffers (own rows +- (radius + 1) * iters), "
                                  "they hold [%d,%d): plan the shard with its iterations (ShardPlan(iters=...))"
                                  % (k, p["iters"], lo, hi, s["buf0"][k], s["buf1"][k]))
        plane_bytes = align_up(s["pitch"][k] * (s["buf1"][k] - s["buf0"][k]) + 64, K_ALIGN)
        plane_bytes_of.append(plane_bytes)
        for t in range(n_sets + 2 + n_iter_sets):
            off_plane[t].append(total)
            total += plane_bytes
        off_flow.append(total)
        own_rows = s["fl1"][k] - s["fl0"][k]
        flow_bytes = align_up((own_rows if own_rows else 1) * s["w"][k] * 2 * 4, K_ALIGN)
        total += flow_bytes
        off_flow2.append(total)
        total += flow_bytes * (B - 1)
        flow_stride.append(flow_bytes)
    # :135-166
    off_patch = [[] for _ in range(K_SETS)]
    off_pscr = []
    pscr_frame = 0
    patch_bytes = [0] * MAX_LEVELS
    repair = False
    if p["local_corner"] or p["stream_two_stage"]:
        step = 1 << (L - 1)
        side = p["patch_size"] if p["patch_size"] > 0 else step * ((p["window"] >> 1) + 2 + 8)
        if p["patch_size"] <= 0 and side < 256:
            side = 256
        side = align_up(side, step)
        pw0 = side if side < p["width"] else p["width"]
        ph0 = side if side < p["height"] else p["height"]
        for k in range(L):
            s["pw"][k] = pw0 >> k
            s["ph"][k] = ph0 >> k
            s["ppitch"][k] = align_up(s["pw"][k], 64)
            patch_bytes[k] = align_up(s["ppitch"][k] * s["ph"][k] + 64, K_ALIGN)
        need = (p["window"] >> 1) + 2
        lc = L - 1
        if s["pw"][lc] < (need if need < s["w"][lc] else s["w"][lc]) or s["ph"][lc] < (need if need < s["h"][lc] else s["h"][lc]):
            raise LayoutError("ofx_session_create: patch_size %d leaves %dx%d at the coarsest level, the corner needs %d"
                              % (side, s["pw"][lc], s["ph"][lc], need))
        need_r = (p["window"] >> 1) + 5
        room = (s["pw"][lc] >= need_r or s["pw"][lc] >= s["w"][lc]) and (s["ph"][lc] >= need_r or s["ph"][lc] >= s["h"][lc])
        repair = bool(p["borrow_frames"] and not p["frames_partial"] and L >= 3 and room)
    # :167-187
    debug_extent = 0
    if repair:
        debug_extent = e["OFX_DEBUG_CORNER_EXTENT"] if e["OFX_DEBUG_CORNER_EXTENT"] is not None else 0
    frames_per_slot = (2 if p["stream_two_stage"] else 0) + (1 if repair else 0)
    if p["local_corner"] or p["stream_two_stage"]:
        for k in range(L):
            off_pscr.append(pscr_frame)
            if k >= 1:
                pscr_frame += patch_bytes[k]
            if p["stream_two_stage"]:
                continue
            for t in range(n_sets):
                off_patch[t].append(total)
                total += patch_bytes[k]
        off_pscr_base = total
        total += pscr_frame * frames_per_slot * B
        off_pscr = [o + off_pscr_base for o in off_pscr]
    # :188-198
    off_status = total
    total += align_up(4 * (1 + K_UV_SLOTS), K_ALIGN)
    off_uv = total
    total += align_up(MAX_LEVELS * 2 * 4 * K_UV_SLOTS, K_ALIGN)
    off_staging = total
    if not p["sharded"]:
        total += align_up(p["width"] * p["height"] * 3, K_ALIGN)
    for k in range(L):
        off_flow_alt.append(total)
        if want_pairs:
            total += flow_stride[k] * B
    # :214-240: the pointers (base + ...)
    at = {}
    for k in range(L):
        for t in range(n_sets):
            at["img", t, 0, k] = off_plane[t][k]
        for t in range(2):
            at["sh", t, 0, k] = off_plane[n_sets + t][k]
        for t in range(n_iter_sets):
            at["itsh", t // 3, t % 3, k] = off_plane[n_sets + 2 + t][k]
        at["flowset", 0, 0, k] = off_flow[k]
        for t in range(1, K_MAX_BATCH):
            at["flowset", t, 0, k] = off_flow2[k] + (t - 1) * flow_stride[k] if t < p["stream_batch"] else off_flow[k]
        if want_pairs:
            for t in range(B):
                at["flowset2", t, 0, k] = off_flow_alt[k] + t * flow_stride[k]
    if p["local_corner"] and not p["stream_two_stage"]:
        for k in range(L):
            for t in range(n_sets):
                at["pimg", t, 0, k] = off_patch[t][k]
    if frames_per_slot > 0:
        for i in range(B):
            for k in range(1, L):
                slot = off_pscr[k] + (frames_per_slot * i) * pscr_frame
                if p["stream_two_stage"]:
                    at["pscr", i, 0, k] = slot
                    at["pscr", i, 1, k] = slot + pscr_frame
                if repair:
                    at["preloc", i, 0, k] = slot + (frames_per_slot - 1) * pscr_frame
    at["status", 0, 0, 0] = off_status
    at["uv", 0, 0, 0] = off_uv
    if not p["sharded"]:
        at["staging", 0, 0, 0] = off_staging
    # :241-252
    fused_iters = p["iters"] > 1 and (e["OFX_ITER_FUSED"] is None or e["OFX_ITER_FUSED"] != 0)
    if (s["buf1"][0] - s["buf0"][0]) * s["pitch"][0] >= (1 << 31) or (s["buf1"][0] - s["buf0"][0]) * s["w"][0] * 8 >= (1 << 31):
        fused_iters = False
    iter_pairs = want_pairs and fused_iters
    pair_pack = 1 if (e["OFX_PAIR_PACK"] is None or e["OFX_PAIR_PACK"] != 0) else 0
    pair_waves = e["OFX_PAIR_WAVES"] if (e["OFX_PAIR_WAVES"] is not None and e["OFX_PAIR_WAVES"] > 0) else 0
    out = dict(s)
    out.update(B=B, n_sets=n_sets, n_iter_sets=n_iter_sets, frames_per_slot=frames_per_slot, repair=int(repair), debug_extent=debug_extent,
               fused_iters=int(fused_iters), iter_pairs=int(iter_pairs), pair_pack=pair_pack, pair_waves=pair_waves, pscr_frame=pscr_frame,
               borrow_frames=p["borrow_frames"], stream_two_stage=p["stream_two_stage"], total=total,
               plane_bytes=plane_bytes_of, flow_bytes=flow_stride, patch_bytes=patch_bytes[:L], at=at)
    return out
