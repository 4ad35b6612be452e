"""What an LK launch did before csrc/lk_plan.h held the decision: a transcription, function by function, of the host code that chose the
kernel variant, the deep fetch, the strips and the wave count -- lk_dispatch and the tail of ofx_stream_launch (lk_level.hip),
plan_table_g, lk_wave_target, launch_iter_r, launch_stream_r and launch_stream_rd (lk_launch.h), and the radius dispatch of the
families (lk_inst.h) -- as they stood in the commit before the header.  tests/test_lk_plan.py compares the header with it.

An item is a dict of the fields of an LkArgs that the code read: w, h, pitch, row0, row_end, out_y0, out_y1, flow_row0, accumulate,
warp_out (bool: the pointer is set).  env maps a switch's name to the int that atoi made of it, or None (not set)."""
from collections import Counter

E_INVALID, E_UNSUPPORTED = 1, 3
COMPAT_CPU, LK_FLOAT, LK_FLOAT_FAST = 0, 1, 2
ENV = dict(OFX_LK_DMA=None, OFX_ITER_DMA=None, OFX_LK_MIN_STRIP=None, OFX_LK_WAVES_PER_SIMD=None, OFX_LK_FILL=None, OFX_LK_TARGET_WAVES=None)


class Rejected(Exception):
    def __init__(self, code, message):
        super().__init__(message)
        self.code = code


def div_up(a, b):
    return (a + b - 1) // b


def env_int(env, name, dflt):
    """lk_launch.h: env_int"""
    v = env.get(name)
    return v if v is not None and v > 0 else dflt


def deep_fetch_by_size(px):
    """session_plan.h"""
    return px >= 16 * 1000 * 1000


def fits_buffer_offsets(a):
    """lk_level.hip, on session_plan.h's"""
    return (a["row_end"] - a["row0"]) * a["pitch"] < (1 << 31) and (a["out_y1"] - a["flow_row0"]) * a["w"] * 8 < (1 << 31)


def plan_table(items, out_w, capacity, env):
    """plan_table_g: (strip_h, tiles_x, first_block) per item, the common strip height and the block count.  (The sum over the items
    is taken per distinct (w, rows_out) with its count: a launch of 80 items has six.)"""
    min_h = env_int(env, "OFX_LK_MIN_STRIP", 8)
    rows_out = [a["out_y1"] - a["out_y0"] for a in items]   # (lk_build_levels)
    max_rows = max([1] + rows_out)

    def height(rows, H):
        hi = min_h if H < min_h else H
        return hi if hi < rows else rows

    kinds = Counter((a["w"], r) for a, r in zip(items, rows_out))
    strip_h = min_h
    while strip_h < max_rows:
        waves = sum(c * div_up(w, out_w) * div_up(r, height(r, strip_h)) for (w, r), c in kinds.items())
        if waves <= capacity:
            break
        strip_h += 1
    t = dict(H=strip_h, tiles_x=[], strip_h=[], first_block=[])
    blocks = 0
    for a, r in zip(items, rows_out):
        t["tiles_x"].append(div_up(a["w"], out_w))
        t["strip_h"].append(height(r, strip_h))
        t["first_block"].append(blocks)
        blocks += t["tiles_x"][-1] * div_up(r, t["strip_h"][-1])
    t["first_block"].append(blocks)
    t["blocks"] = blocks
    return t


def wave_target(cus, occ, reserve, dflt_per_simd, full_fill, env):
    """lk_wave_target after its HIP queries: cus = multiProcessorCount, occ = per_cu * (threads / 64) / 4"""
    per_simd = env_int(env, "OFX_LK_WAVES_PER_SIMD", dflt_per_simd)
    if per_simd > occ - reserve:
        per_simd = occ - reserve
    if per_simd < 1:
        per_simd = 1
    fill = env_int(env, "OFX_LK_FILL", 100 if per_simd < occ else full_fill)
    return env_int(env, "OFX_LK_TARGET_WAVES", cus * 4 * per_simd * fill // 100)


# (reserve, dflt_per_simd, full_fill) of the call sites: launch_r and launch_iter_rd, launch_pair_r, launch_stream_rd's capacity1 / capacity2
CALL_SITES = {"levels": (0, 4, 95), "pair": (0, 2, 100), "tick_one": (1, 2, 95), "tick_many": (1, 4, 95)}


def check_radius(radius, kernel_mode, what="ofx_lk_level"):
    """dispatch_radius<lk_max_radius(MODE)> in lk_inst.h"""
    if not 1 <= radius <= (12 if kernel_mode == COMPAT_CPU else 11):
        raise Rejected(E_UNSUPPORTED, "%s: window %d not supported in mode %d" % (what, 2 * radius + 1, kernel_mode))


def variant(family, mode, fast=False, sums=False, iter=0, deep=False, many=False):
    return dict(family=family, mode=mode, fast=int(fast), sums=int(sums), iter=iter, deep=int(deep), many=int(many))


def levels_variant(items, radius, mode, sums, env):
    """lk_dispatch after lk_build_levels, down to the kernel: ofx_launch::levels / iter, launch_iter_r"""
    lv0 = items[0]
    if (lv0["accumulate"] or lv0["warp_out"]) and not sums:
        small = all(fits_buffer_offsets(a) for a in items)
        wout = bool(lv0["warp_out"])
        if not (not wout or (small and mode != COMPAT_CPU)):
            raise Rejected(E_INVALID, "ofx_lk_levels: d_warp_out needs mode lk_float and levels below 2 GB")
        rowwin = any(a["row0"] != 0 or a["row_end"] != a["h"] for a in items)
        if wout and rowwin and not lv0["accumulate"]:
            raise Rejected(E_INVALID, "ofx_lk_levels: iteration 1 with d_warp_out on a row window runs in the stream tick only")
        it = ((4 if rowwin else 2) if lv0["accumulate"] else 3) if wout else 1
        if small and mode != COMPAT_CPU:
            check_radius(radius, LK_FLOAT)
            forced = env.get("OFX_ITER_DMA")
            forced = -1 if forced is None else forced
            max_px = max(a["w"] * a["h"] for a in items)
            deep = forced > 0 or (forced < 0 and deep_fetch_by_size(max_px))
            return variant("iter", LK_FLOAT, mode == LK_FLOAT_FAST, False, it, deep)
    if mode == COMPAT_CPU:
        check_radius(radius, COMPAT_CPU)
        return variant("levels", COMPAT_CPU, False, sums)
    check_radius(radius, LK_FLOAT)
    if mode == LK_FLOAT_FAST and not sums:
        return variant("levels", LK_FLOAT, True, False)
    return variant("levels", LK_FLOAT, False, sums)


def tick_variant(items, mode, hint, env):
    """the tail of ofx_stream_launch, launch_stream_r and the capacity choice of launch_stream_rd"""
    kernel_mode, fast, wout = COMPAT_CPU, False, 0
    if mode != COMPAT_CPU:
        kernel_mode, fast = LK_FLOAT, mode == LK_FLOAT_FAST
        if items and items[0]["warp_out"]:
            wout = 5 if any(a["row0"] != 0 or a["row_end"] != a["h"] for a in items) else 3
    deep = False
    if not wout:
        forced = env.get("OFX_LK_DMA")
        forced = -1 if forced is None else forced
        max_px = max([0] + [a["w"] * a["h"] for a in items])
        want = (1 if forced > 0 else -1) if forced >= 0 else hint
        deep = want > 0 or (want == 0 and deep_fetch_by_size(max_px))
    pairs = sum(1 for a in items if a["w"] == items[0]["w"] and a["h"] == items[0]["h"])
    return variant("stream", kernel_mode, fast, False, wout, deep, pairs >= 2)
