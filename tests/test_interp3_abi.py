"""CPU: the colour interpolation calls (ofx_interpolate_frames_3ch, ofx_interpolate_frames_3ch_batch) are declared in include/ofx.h,
exported by the library and bound in lib.py with the header's argument lists; bad sizes, pitches (compared against 3 * w),
alignments, times, strides and batch arrays are refused with OFX_E_INVALID before anything is enqueued; the engine has its three new
functions; the ABI version and the timing kinds did not move.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ofx_interpolate_frames_3ch", "ofx_interpolate_frames_3ch_batch"]
OFX_E_INVALID = 1
NAN, INF = float("nan"), float("inf")


def test_declared_exported_and_bound():
    from cuda_optical_flow_2_amd import build, lib

    build.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ofx_[a-z0-9_]+)\s*\(", text))
    nm = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    L = lib.load()
    for name in CALLS:
        assert name in declared, f"{name} is not declared in include/ofx.h"
        assert name in exported, f"{name} is not exported by the library"
        assert name in lib.EXPORTS and name in lib._SIGS, f"{name} is not in lib.EXPORTS / lib._SIGS"
        assert getattr(L, name).argtypes == lib._SIGS[name]
    # the bound argument lists are the header's: as many arguments, floats, ints and sizes where it has them
    for name in CALLS:
        args = re.search(name + r"\s*\(([^;]*)\)\s*;", text).group(1).split(",")
        assert len(args) == len(lib._SIGS[name]) == 16 - (name == CALLS[0]), name
        for decl, bound in zip(args, lib._SIGS[name]):
            assert (bound is C.c_float) == bool(re.match(r"float\s+\w", decl.strip())), (name, decl)
            assert (bound is C.c_int) == bool(re.match(r"int\s+\w", decl.strip())), (name, decl)
            assert (bound is C.c_size_t) == bool(re.match(r"size_t\s+\w", decl.strip())), (name, decl)
    # ... and the grey calls' own, argument for argument
    assert lib._SIGS[CALLS[0]] == lib._SIGS["ofx_interpolate_frames"] and lib._SIGS[CALLS[1]] == lib._SIGS["ofx_interpolate_frames_batch"]


def test_python_surface_and_the_definition():
    from cuda_optical_flow_2_amd import engine

    for name in ("interpolate_frames_colour", "video_interpolate_colour", "video_interpolate_colour_dense"):
        assert callable(getattr(engine, name))
    text = open(os.path.join(ROOT, "include", "ofx.h")).read()
    assert "---- colour frame interpolation" in text and text.index("---- colour frame interpolation") > text.index("---- frame interpolation")


def _times(*values):
    return (C.c_float * len(values))(*values)


def test_the_call_refuses_bad_arguments_before_it_enqueues_anything():
    """The addresses are never dereferenced: every case below fails a check on the host."""
    from cuda_optical_flow_2_amd import lib

    L = lib.load()
    A, B, AB, BA, D, S = 0x10001, 0x20002, 0x30000, 0x40000, 0x50003, 0x60000     # (planes and frames need no alignment)
    w, h = 64, 8
    T3 = _times(0.25, 0.5, 0.75)

    def call(a=A, ap=192, b=B, bp=200, w=w, h=h, ab=AB, ba=BA, times=T3, nt=3, dst=D, dp=192, ts=192 * 8, stats=S):
        return L.ofx_interpolate_frames_3ch(a, ap, b, bp, w, h, ab, ba, times, nt, dst, dp, ts, stats, None)

    for kw, word in ((dict(a=None), b"d_a3"), (dict(b=None), b"d_b3"), (dict(ab=None), b"d_disp_ab"), (dict(ba=None), b"d_disp_ba"),
                     (dict(dst=None), b"d_dst3"), (dict(times=None), b"h_times")):
        assert call(**kw) == OFX_E_INVALID, kw
        assert word in L.ofx_last_error(), kw
    assert call(w=0) == OFX_E_INVALID and call(h=0) == OFX_E_INVALID and call(w=-4) == OFX_E_INVALID and call(h=-1) == OFX_E_INVALID
    big = dict(ap=3 << 14, bp=3 << 14, dp=3 << 14, ts=3 << 28)
    assert call(w=1 << 14, h=1 << 14, **big) == OFX_E_INVALID                 # 2^28 pixels
    assert b"w * h" in L.ofx_last_error()
    # a pitch below a row's 3 * w bytes: one short, and one that would do for a grey plane
    for kw in (dict(ap=191), dict(bp=191), dict(dp=191), dict(ap=64), dict(bp=100), dict(dp=64, ts=1 << 20), dict(ap=0), dict(bp=-192)):
        assert call(**kw) == OFX_E_INVALID, kw
        assert b"pitch" in L.ofx_last_error(), kw
    # a plane of 2^31 bytes or more: 2^13 rows, 2^18 bytes apart (w * h = 2^19 pixels only)
    for kw in (dict(ap=1 << 18), dict(bp=1 << 18)):
        assert call(h=1 << 13, ts=1 << 30, **kw) == OFX_E_INVALID, kw
        assert b"2^31" in L.ofx_last_error(), kw
    for kw in (dict(ab=AB + 4), dict(ba=BA + 4), dict(stats=S + 4)):
        assert call(**kw) == OFX_E_INVALID, kw
        assert b"aligned" in L.ofx_last_error(), kw
    for nt in (0, 9, -1):
        assert call(times=_times(*[0.5] * 9), nt=nt) == OFX_E_INVALID, nt
        assert b"n_times" in L.ofx_last_error()
    for bad in (NAN, INF, -INF, 0.0, 1.0, -0.25, 1.5):
        assert call(times=_times(0.25, bad, 0.75)) == OFX_E_INVALID, bad
        assert b"h_times" in L.ofx_last_error()
    assert call(ts=192 * 8 - 1) == OFX_E_INVALID                               # frames would overlap
    assert b"time_stride_bytes" in L.ofx_last_error()
    assert call(dp=200, ts=192 * 8) == OFX_E_INVALID
    assert call(ts=64 * 8) == OFX_E_INVALID                                    # a grey frame's stride


def test_the_batch_call_refuses_bad_arguments_before_it_enqueues_anything():
    from cuda_optical_flow_2_amd import lib

    L = lib.load()
    vp = C.c_void_p

    def arr(base, n=17, hole=None, step=0x100000):
        return (vp * n)(*[None if i == hole else base + i * step for i in range(n)])

    def ints(v, n=17):
        return (C.c_int * n)(*[v] * n)

    A, B, AB, BA, D, S = arr(0x10000001), arr(0x20000002), arr(0x30000000), arr(0x40000000), arr(0x50000003), arr(0x60000000)
    w, h = 64, 8
    T3 = _times(0.25, 0.5, 0.75)

    def call(a=A, ap=ints(192), b=B, bp=ints(200), n=3, w=w, h=h, ab=AB, ba=BA, times=T3, nt=3, dst=D, dp=192, ts=192 * 8, stats=S):
        return L.ofx_interpolate_frames_3ch_batch(a, ap, b, bp, n, w, h, ab, ba, times, nt, dst, dp, ts, stats, None)

    for n in (0, 17, -1):
        assert call(n=n) == OFX_E_INVALID, n
        assert b"n = " in L.ofx_last_error()
    for kw, word in (("a", b"d_a3"), ("ap", b"a_pitches"), ("b", b"d_b3"), ("bp", b"b_pitches"), ("ab", b"d_disp_ab"), ("ba", b"d_disp_ba"),
                     ("dst", b"d_dst3"), ("times", b"h_times")):                # a null array
        assert call(**{kw: None}) == OFX_E_INVALID, kw
        assert word in L.ofx_last_error(), kw
    for kw in ("a", "b", "ab", "ba", "dst", "stats"):                           # a NULL entry in a non-NULL array
        assert call(**{kw: arr(0x70000000, hole=2)}) == OFX_E_INVALID, kw
        assert b"pair 2" in L.ofx_last_error(), kw
    for short in (191, 64):                                                     # one pair's pitch, not the first
        bad_pitch = ints(192)
        bad_pitch[1] = short
        for kw in (dict(ap=bad_pitch), dict(bp=bad_pitch), dict(dp=short, ts=1 << 20)):
            assert call(**kw) == OFX_E_INVALID, (short, kw)
            assert b"pitch" in L.ofx_last_error(), (short, kw)
    huge = ints(192)
    huge[2] = 1 << 18
    assert call(h=1 << 13, ts=1 << 30, ap=huge) == OFX_E_INVALID and b"2^31" in L.ofx_last_error()
    for kw in ("ab", "ba", "stats"):                                            # one misaligned entry, not the first
        a = arr(0x70000000)
        a[1] = 0x70000000 + 0x100000 + 4
        assert call(**{kw: a}) == OFX_E_INVALID, kw
        assert b"aligned" in L.ofx_last_error(), kw
    assert call(w=1 << 14, h=1 << 14, ap=ints(3 << 14), bp=ints(3 << 14), dp=3 << 14, ts=3 << 28) == OFX_E_INVALID
    assert b"w * h" in L.ofx_last_error()
    assert call(nt=0) == OFX_E_INVALID and call(times=_times(*[0.5] * 9), nt=9) == OFX_E_INVALID
    assert b"n_times" in L.ofx_last_error()
    assert call(times=_times(0.25, NAN, 0.75)) == OFX_E_INVALID and call(times=_times(0.0, 0.5, 0.75)) == OFX_E_INVALID
    assert call(times=_times(0.25, 0.5, 1.0)) == OFX_E_INVALID
    assert b"h_times" in L.ofx_last_error()
    assert call(ts=192 * 8 - 8) == OFX_E_INVALID
    assert b"time_stride_bytes" in L.ofx_last_error()


def test_abi_version_and_timing_kinds_did_not_move():
    from cuda_optical_flow_2_amd import engine, lib

    assert lib.load().ofx_abi_version() == 10
    text = open(os.path.join(ROOT, "include", "ofx.h")).read()
    assert re.search(r"#define\s+OFX_TIME_KINDS\s+9\b", text)
    assert len(engine.Session.TIME_KINDS) == 9
