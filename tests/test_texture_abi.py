"""CPU: the texture calls (ofx_texture_features, ofx_compact_features) are declared in include/ofx.h, exported by the library and
bound in lib.py; the header compiles as C and as C++ and ofx_texture_desc has the layout of its ctypes twin; ofx_params, the ABI
version and the timing kinds did not move; both calls refuse bad arguments with OFX_E_INVALID and a message that names the item,
before anything is enqueued.  No compute calls."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ofx_texture_features", "ofx_compact_features"]
OFX_E_INVALID = 1
OFX_STREAM_MAX_BATCH = 16
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
    assert lib._SIGS["ofx_texture_features"] == [C.POINTER(lib.TextureDesc), C.c_int, C.c_int, C.c_void_p]
    assert lib._SIGS["ofx_compact_features"] == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert "texture.hip" in build.SOURCES and not any("corner" in s for s in build.SOURCES if "texture" in s)


def test_python_surface():
    from cuda_optical_flow_2_amd import engine

    assert list(inspect.signature(engine.texture_strength).parameters) == ["img", "window"]
    p = inspect.signature(engine.good_features).parameters
    assert list(p) == ["img", "window", "cell", "border", "min_strength", "max_points"]
    assert p["cell"].default == 16 and p["border"].default is None and p["min_strength"].default == 0.0 and p["max_points"].default is None
    p = inspect.signature(engine.video_tracks_auto).parameters
    assert list(p)[:5] == ["frames", "levels", "window", "cell", "level"] and p["cell"].default == 16 and p["level"].default == 0


@pytest.mark.parametrize("cc,flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_the_header_compiles_and_the_struct_has_the_bound_layout(tmp_path, cc, flags):
    from cuda_optical_flow_2_amd import lib

    fields = [f[0] for f in lib.TextureDesc._fields_]
    assert fields == ["d_plane", "pitch", "w", "h", "d_strength", "strength_pitch", "d_cells", "d_cell_strength", "d_stats", "cell", "border",
                      "min_strength"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ofx.h"\n'
           'int main(void){ofx_texture_desc d; (void)d; printf("%zu %zu", sizeof(ofx_texture_desc), sizeof(ofx_params));\n'
           + "".join(f'printf(" %zu", offsetof(ofx_texture_desc, {f}));\n' for f in fields) + 'printf("\\n"); return 0;}\n')
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = tmp_path / "t"
    subprocess.run([cc, "-Wall", "-Werror"] + flags + [str(c), "-I", os.path.join(ROOT, "include"), "-o", str(exe)], check=True)
    size, params, *offs = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == C.sizeof(lib.TextureDesc)
    assert offs == [getattr(lib.TextureDesc, f).offset for f in fields]
    assert params == C.sizeof(lib.Params), "sizeof(ofx_params) moved"


def test_abi_version_params_and_timing_kinds_did_not_move():
    from cuda_optical_flow_2_amd import engine, lib

    assert lib.load().ofx_abi_version() == 10
    text = open(os.path.join(ROOT, "include", "ofx.h")).read()
    assert re.search(r"#define\s+OFX_TIME_KINDS\s+9\b", text)
    assert re.search(r"#define\s+OFX_STREAM_MAX_BATCH\s+16\b", text)
    assert len(engine.Session.TIME_KINDS) == 9
    assert C.sizeof(lib.Params) == 352


def test_texture_features_refuses_bad_descriptors_before_it_enqueues_anything():
    """The addresses are never dereferenced: every case below fails a check on the host."""
    from cuda_optical_flow_2_amd import lib

    L = lib.load()
    PL, ST, CE, CS, SS = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000   # made-up, suitably aligned addresses
    NB = OFX_STREAM_MAX_BATCH

    def desc(plane=PL, pitch=40, w=40, h=12, strength=ST, sp=40, cells=CE, cs=CS, stats=SS, cell=16, border=5, thr=0.0):
        return lib.TextureDesc(plane, pitch, w, h, strength, sp, cells, cs, stats, cell, border, thr)

    def refused(word, n=1, window=9, **kw):
        d = (lib.TextureDesc * NB)(*[desc() for _ in range(NB)])
        at = max(min(n, NB), 1) - 1
        d[at] = desc(**kw)                                        # the bad one is the last of the launch
        rc = L.ofx_texture_features(d, n, window, None)
        msg = L.ofx_last_error()
        assert rc == OFX_E_INVALID, (kw, n, window, rc)
        assert msg and word in msg, (kw, n, window, msg)
        if kw:
            assert b"item %d" % at in msg, (kw, n, msg)

    for n in (1, 3, NB):
        for kw in (dict(plane=None), dict(strength=None)):
            refused(b"null", n, **kw)
        for kw in (dict(w=0), dict(h=0), dict(w=-3), dict(h=-1)):
            refused(b"positive", n, **kw)
        for kw in (dict(w=1 << 14, h=1 << 14, pitch=1 << 14, sp=1 << 14), dict(w=1 << 20, h=1 << 10, pitch=1 << 20, sp=1 << 20)):
            refused(b"2^28", n, **kw)                             # w * h >= 2^28
        for kw in (dict(pitch=36), dict(pitch=0), dict(pitch=-40), dict(pitch=42), dict(w=41, pitch=41, sp=41)):
            refused(b"pitch", n, **kw)                            # below the width, or no multiple of 4
        refused(b"2^31", n, w=1 << 10, h=1 << 10, pitch=1 << 21, sp=1 << 10)
        for kw in (dict(sp=39), dict(sp=0), dict(sp=-40)):
            refused(b"strength_pitch", n, **kw)
        for kw in (dict(plane=PL + 1), dict(plane=PL + 2), dict(strength=ST + 2), dict(cells=CE + 2), dict(cs=CS + 1), dict(stats=SS + 4)):
            refused(b"aligned", n, **kw)
        for cell in (3, 0, -16, 257, 1 << 20):
            refused(b"cell", n, cell=cell)
        for border in (-1, -100):
            refused(b"border", n, border=border)
        for thr in (NAN, INF, -INF, -1.0, -1e-30):
            refused(b"min_strength", n, thr=thr)
        refused(b"go together", n, cells=None)
        refused(b"go together", n, cs=None)
        refused(b"d_stats without", n, cells=None, cs=None)
        for window in (8, 2, 1, 0, -3, 25, 24, 4):
            refused(b"window", n, window=window)
    for n in (0, -1, NB + 1, 1 << 20):
        refused(b"n = ", n)
    assert L.ofx_texture_features(None, 1, 9, None) == OFX_E_INVALID and b"null" in L.ofx_last_error()
    # what is allowed passes the checks of the items BEFORE a refused one: a strength-only item (its cell, border and min_strength
    # are not looked at), cells without stats, the smallest and the largest cell, a border larger than the plane, odd sizes
    d = (lib.TextureDesc * 5)(desc(cells=None, cs=None, stats=None, cell=0, border=-1, thr=NAN), desc(stats=None, cell=4), desc(cell=256, border=1000),
                              desc(w=37, h=5, pitch=40, sp=37, thr=1e30), desc(cell=3))
    assert L.ofx_texture_features(d, 5, 23, None) == OFX_E_INVALID and b"item 4" in L.ofx_last_error()


def test_compact_features_refuses_bad_arguments_before_it_enqueues_anything():
    from cuda_optical_flow_2_amd import lib

    L = lib.load()
    CE, PT, CN = 0x30000000, 0x40000000, 0x50000000

    def refused(word, cells=CE, n_cells=12, max_points=5, points=PT, count=CN):
        rc = L.ofx_compact_features(cells, n_cells, max_points, points, count, None)
        msg = L.ofx_last_error()
        assert rc == OFX_E_INVALID and msg and word in msg, (rc, msg)

    refused(b"null", cells=None)
    refused(b"null", count=None)
    refused(b"null", points=None)
    for n_cells in (0, -1, 1 << 28):
        refused(b"n_cells", n_cells=n_cells)
    refused(b"max_points", max_points=-1)
    for kw in (dict(cells=CE + 2), dict(points=PT + 1), dict(count=CN + 2)):
        refused(b"aligned", **kw)
