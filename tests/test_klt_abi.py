"""CPU: ofx_track_points is declared in include/ofx.h, exported by the library and bound in lib.py; the header compiles as C and as
C++ and ofx_track_clip / ofx_track_params have the layouts of their ctypes twins; ofx_params, the ABI version and the timing kinds
did not move; the call refuses bad arguments with OFX_E_INVALID and a message that names the argument, before anything is enqueued.
No compute calls."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    name = "ofx_track_points"
    assert name in declared, f"{name} is not declared in include/ofx.h"
    assert name in exported, f"{name} is not exported by the library"
    assert name in lib.EXPORTS and name in lib._SIGS, f"{name} is not in lib.EXPORTS / lib._SIGS"
    assert getattr(L, name).argtypes == lib._SIGS[name]
    vp = C.c_void_p
    assert lib._SIGS[name] == [C.POINTER(lib.TrackClip), C.POINTER(lib.TrackParams), C.c_int, vp, vp, C.c_int, vp, vp, vp, vp]
    assert "klt.hip" in build.SOURCES
    for word, value in (("OFX_TRACK_START", 1), ("OFX_TRACK_SINGULAR", 2), ("OFX_TRACK_OUT", 3), ("OFX_TRACK_RESIDUAL", 4), ("OFX_TRACK_MAX_LEVELS", 8)):
        assert re.search(rf"#define\s+{word}\s+{value}\b", text)


def test_python_surface():
    from cuda_optical_flow_2_amd import engine

    p = inspect.signature(engine.track_points).parameters
    assert list(p) == ["prev", "next", "points", "levels", "window", "max_iters", "eps", "min_lambda", "max_sad", "fb_max"]
    assert p["max_iters"].default == 10 and p["eps"].default == 1 / 32 and p["min_lambda"].default == 0.0 and p["max_sad"].default == 0
    assert p["fb_max"].default is None
    p = inspect.signature(engine.video_klt).parameters
    assert list(p)[:6] == ["frames", "points", "levels", "window", "cell", "batch"]
    assert p["points"].default is None and p["cell"].default == 16 and p["batch"].default == 16
    assert (engine.TRACK_START, engine.TRACK_SINGULAR, engine.TRACK_OUT, engine.TRACK_RESIDUAL, engine.TRACK_FB) == (1, 2, 3, 4, 5)


@pytest.mark.parametrize("cc,flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_the_header_compiles_and_the_structs_have_the_bound_layouts(tmp_path, cc, flags):
    from cuda_optical_flow_2_amd import lib

    clip = [f[0] for f in lib.TrackClip._fields_]
    prm = [f[0] for f in lib.TrackParams._fields_]
    assert clip == ["w", "h", "levels", "n_frames", "planes", "pitches"] and prm == ["window", "max_iters", "eps_q", "max_sad", "min_lambda"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ofx.h"\n'
           'int main(void){ofx_track_clip c; ofx_track_params p; (void)c; (void)p;\n'
           'printf("%zu %zu %zu", sizeof(ofx_track_clip), sizeof(ofx_track_params), sizeof(ofx_params));\n'
           + "".join(f'printf(" %zu", offsetof(ofx_track_clip, {f}));\n' for f in clip)
           + "".join(f'printf(" %zu", offsetof(ofx_track_params, {f}));\n' for f in prm) + 'printf("\\n"); return 0;}\n')
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = tmp_path / "t"
    subprocess.run([cc, "-Wall", "-Werror"] + flags + [str(c), "-I", os.path.join(ROOT, "include"), "-o", str(exe)], check=True)
    s_clip, s_prm, params, *offs = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert s_clip == C.sizeof(lib.TrackClip) and s_prm == C.sizeof(lib.TrackParams)
    assert offs == [getattr(lib.TrackClip, f).offset for f in clip] + [getattr(lib.TrackParams, f).offset for f in prm]
    assert params == C.sizeof(lib.Params), "sizeof(ofx_params) moved"


def test_abi_version_params_and_timing_kinds_did_not_move():
    from cuda_optical_flow_2_amd import engine, lib

    assert lib.load().ofx_abi_version() == 10
    text = open(os.path.join(ROOT, "include", "ofx.h")).read()
    assert re.search(r"#define\s+OFX_TIME_KINDS\s+9\b", text)
    assert re.search(r"#define\s+OFX_STREAM_MAX_BATCH\s+16\b", text)
    assert len(engine.Session.TIME_KINDS) == 9
    assert C.sizeof(lib.Params) == 352


def test_track_points_refuses_bad_arguments_before_it_enqueues_anything():
    """The addresses are never dereferenced: every case below fails a check on the host."""
    from cuda_optical_flow_2_amd import lib

    L = lib.load()
    PL, PT, ST, HI, SA, SS = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000   # made-up addresses

    def call(w=64, h=48, levels=3, n_frames=3, planes="ok", pitches="ok", window=9, max_iters=10, eps_q=1, max_sad=0, min_lambda=0.0, pair0=1,
             points=PT, status=ST, n=10, history=HI, sad=SA, stats=SS, clip="ok", prm="ok", null_plane=None, odd_plane=False):
        nl, nf = max(min(levels, 8), 1), max(min(n_frames, 17), 2)
        table = (C.c_void_p * (nf * nl))(*[PL + 0x100000 * i + (1 if odd_plane else 0) for i in range(nf * nl)])
        if null_plane is not None:
            table[null_plane] = None
        pt = (C.c_int * nl)(*(pitches if isinstance(pitches, list) else [(w >> k) + (k & 1) for k in range(nl)]))
        c = lib.TrackClip(w, h, levels, n_frames, table if planes == "ok" else None, pt if pitches is not None else None)
        p = lib.TrackParams(window, max_iters, eps_q, max_sad, min_lambda)
        rc = L.ofx_track_points(C.byref(c) if clip == "ok" else None, C.byref(p) if prm == "ok" else None, pair0, points, status, n, history, sad, stats, None)
        return rc, L.ofx_last_error()

    def refused(word, **kw):
        rc, msg = call(**kw)
        assert rc == OFX_E_INVALID, (kw, rc)
        assert msg and word in msg, (kw, msg)

    for kw in (dict(clip=None), dict(prm=None), dict(planes=None), dict(pitches=None), dict(points=None), dict(status=None), dict(null_plane=0),
               dict(null_plane=8)):
        refused(b"null", **kw)
    for levels in (0, -1, 9, 100):
        refused(b"levels", levels=levels)
    for kw in (dict(w=3, levels=3), dict(h=7, levels=4), dict(w=0, levels=1), dict(h=-5, levels=1), dict(w=127, h=127, levels=8)):
        refused(b"coarsest", **kw)
    for kw in (dict(w=(1 << 19) + 1, pitches=[1 << 20, 1 << 19, 1 << 18]), dict(h=(1 << 19) + 2)):
        refused(b"2^19", **kw)
    for n_frames in (1, 0, -2, 18, 1 << 20):
        refused(b"n_frames", n_frames=n_frames)
    for window in (8, 2, 1, 0, -3, 25, 24, 4):
        refused(b"window", window=window)
    for it in (0, -1, 33, 1000):
        refused(b"max_iters", max_iters=it)
    refused(b"eps_q", eps_q=-1)
    for v in (NAN, INF, -INF, -1.0, -1e-30):
        refused(b"min_lambda", min_lambda=v)
    refused(b"max_sad", max_sad=-1)
    for kw in (dict(pair0=0), dict(pair0=-1), dict(pair0=(1 << 23) - 2), dict(pair0=(1 << 23) - 16, n_frames=17), dict(pair0=(1 << 31) - 1)):
        refused(b"pair0", **kw)
    for n in (0, -1):
        refused(b"n_points", n=n)
    for pitches in ([63, 32, 16], [64, 31, 16], [64, 32, 15], [0, 32, 16], [-64, 32, 16]):
        refused(b"pitch", pitches=pitches)
    refused(b"2^31", w=1 << 10, h=1 << 10, levels=1, pitches=[1 << 21])
    for kw in (dict(points=PT + 4), dict(history=HI + 4), dict(points=PT + 1)):
        refused(b"8-byte", **kw)
    for kw in (dict(status=ST + 2), dict(sad=SA + 1)):
        refused(b"4-byte", **kw)
    for kw in (dict(stats=SS + 4), dict(stats=SS + 1)):
        refused(b"d_stats", **kw)
    # what is allowed passes every check up to a refused last one: the limits of each range, odd plane addresses and pitches, no
    # optional output, one level, a coarsest level of one pixel
    for kw in (dict(levels=8, w=128, h=300, n_frames=17, window=23, max_iters=32, eps_q=0, max_sad=1 << 30, min_lambda=1e30, pair0=(1 << 23) - 17),
               dict(levels=1, w=1, h=1, n_frames=2, window=3, max_iters=1, history=None, sad=None), dict(odd_plane=True, w=1 << 19, h=2, levels=2),
               dict(pitches=[64, 33, 17], n=1 << 30)):
        refused(b"d_stats", stats=SS + 4, **kw)
