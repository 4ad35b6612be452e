"""CPU: the flow-median calls (ofx_flow_median, ofx_session_run_flow_dense_median, ofx_session_dense_median_scratch_bytes) are
declared in include/ofx.h, exported by the library and bound in lib.py; the header compiles as C and as C++ and ofx_median_desc has
the layout of its ctypes twin; ofx_params, the ABI version and the timing kinds did not move; ofx_flow_median refuses bad
descriptors with OFX_E_INVALID and a message before anything is enqueued; and the kernel's selection networks
(csrc/median_net.h) select the median of every 0-1 input (tests/median_net_check.cpp).  No compute calls."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ofx_flow_median", "ofx_session_run_flow_dense_median", "ofx_session_dense_median_scratch_bytes"]
OFX_E_INVALID = 1
OFX_MAX_LEVELS = 12
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
    assert lib._SIGS["ofx_flow_median"] == [C.POINTER(lib.MedianDesc), C.c_int, C.c_void_p]
    assert lib._SIGS["ofx_session_run_flow_dense_median"] == [C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    assert lib._SIGS["ofx_session_dense_median_scratch_bytes"] == [C.c_void_p, C.POINTER(C.c_size_t)]


def test_python_surface():
    from cuda_optical_flow_2_amd import engine

    sig = inspect.signature(engine.flow_median)
    assert list(sig.parameters) == ["field", "radius", "src", "scale"]
    assert sig.parameters["radius"].default == 2 and sig.parameters["src"].default is None and sig.parameters["scale"].default == engine.ITER_SCALE
    sig = inspect.signature(engine.Session.run_flow_dense)
    assert list(sig.parameters) == ["self", "max_px", "stream", "median"]
    assert sig.parameters["max_px"].default is None and sig.parameters["stream"].default is None and sig.parameters["median"].default == 0
    for name in ("flow_pair_dense", "video_displacement_dense", "video_interpolate_dense", "video_interpolate_colour_dense"):
        p = inspect.signature(getattr(engine, name)).parameters
        assert p["median"].default == 0 and p["median"].annotation in (int, "int"), name


@pytest.mark.parametrize("cc,flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_the_header_compiles_and_the_struct_has_the_bound_layout(tmp_path, cc, flags):
    from cuda_optical_flow_2_amd import lib

    fields = [f[0] for f in lib.MedianDesc._fields_]
    assert fields == ["d_src_flow", "d_dst_flow", "w", "h", "radius", "scale", "d_src", "src_pitch", "d_dst", "dst_pitch"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ofx.h"\n'
           'int main(void){ofx_median_desc d; (void)d; printf("%zu %zu", sizeof(ofx_median_desc), sizeof(ofx_params));\n'
           + "".join(f'printf(" %zu", offsetof(ofx_median_desc, {f}));\n' for f in fields) + 'printf("\\n"); return 0;}\n')
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = tmp_path / "t"
    subprocess.run([cc, "-Wall", "-Werror"] + flags + [str(c), "-I", os.path.join(ROOT, "include"), "-o", str(exe)], check=True)
    size, params, *offs = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == C.sizeof(lib.MedianDesc)
    assert offs == [getattr(lib.MedianDesc, f).offset for f in fields]
    assert params == C.sizeof(lib.Params), "sizeof(ofx_params) moved"


def test_abi_version_params_and_timing_kinds_did_not_move():
    from cuda_optical_flow_2_amd import engine, lib

    assert lib.load().ofx_abi_version() == 10
    text = open(os.path.join(ROOT, "include", "ofx.h")).read()
    assert re.search(r"#define\s+OFX_TIME_KINDS\s+9\b", text)
    assert re.search(r"#define\s+OFX_STREAM_MAX_BATCH\s+16\b", text)
    assert len(engine.Session.TIME_KINDS) == 9
    assert C.sizeof(lib.Params) == 352


def test_median_refuses_bad_descriptors_before_it_enqueues_anything():
    """The addresses are never dereferenced: every case below fails a check on the host."""
    from cuda_optical_flow_2_amd import lib

    L = lib.load()
    FI, FO, SRC, DST = 0x10000000, 0x20000000, 0x30000000, 0x40000000    # made-up, suitably aligned addresses
    NB = OFX_STREAM_MAX_BATCH

    def desc(fin=FI, fout=FO, w=40, h=12, radius=2, scale=0.5, src=SRC, sp=64, dst=DST, dp=64):
        return lib.MedianDesc(fin, fout, w, h, radius, scale, src, sp, dst, dp)

    def refused(word, n=1, **kw):
        d = (lib.MedianDesc * NB)(*[desc() for _ in range(NB)])
        d[max(min(n, NB), 1) - 1] = desc(**kw)                    # the bad one is the last of the launch
        rc = L.ofx_flow_median(d, n, None)
        msg = L.ofx_last_error()
        assert rc == OFX_E_INVALID, (kw, n, rc)
        assert msg and word in msg, (kw, n, msg)

    for n in (1, 3, NB):
        for kw in (dict(fin=None), dict(fout=None)):
            refused(b"null", n, **kw)
        for kw in (dict(w=0), dict(h=0), dict(w=-3), dict(h=-1)):
            refused(b"positive", n, **kw)
        for kw in (dict(w=1 << 14, h=1 << 14, sp=1 << 14, dp=1 << 14), dict(w=1 << 20, h=1 << 10, sp=1 << 20, dp=1 << 20)):
            refused(b"2^28", n, **kw)                             # w * h >= 2^28
        refused(b"2^31", n, w=1 << 10, h=1 << 10, sp=1 << 21, dp=1 << 10)     # a plane of 2^31 bytes
        refused(b"2^31", n, w=1 << 10, h=1 << 10, sp=1 << 10, dp=1 << 21)
        for kw in (dict(sp=39), dict(dp=39), dict(sp=0), dict(dp=-64)):
            refused(b"pitch", n, **kw)
        for kw in (dict(fin=FI + 4), dict(fout=FO + 4), dict(fout=FO + 2)):
            refused(b"aligned", n, **kw)
        # d_dst_flow inside d_src_flow's w * h * 8 bytes, from either side, and in place
        for fout in (FI, FI + 8, FI + 40 * 12 * 8 - 8, FI - 40 * 12 * 8 + 8):
            refused(b"overlaps", n, fout=fout)
        for radius in (0, 3, -1, 5):
            refused(b"radius", n, radius=radius)
        for bad in (NAN, INF, -INF):
            refused(b"scale", n, scale=bad)
        refused(b"d_src and d_dst", n, dst=None)
        refused(b"d_src and d_dst", n, src=None)
        for dst in (SRC, SRC + 11 * 64 + 39, SRC - 11 * 64 - 39, SRC + 4):
            refused(b"overlaps", n, dst=dst)
    for n in (0, -1, NB + 1, 1 << 20):
        refused(b"n = ", n)
    assert L.ofx_flow_median(None, 1, None) == OFX_E_INVALID and b"null" in L.ofx_last_error()
    # fields that touch without overlapping, both radii, odd sizes and a flow-only item pass the checks of items BEFORE a refused one
    d = (lib.MedianDesc * 4)(desc(w=41, h=13, sp=41, dp=41, radius=1), desc(src=None, dst=None, sp=0, dp=0), desc(fout=FI + 40 * 12 * 8),
                             desc(radius=7))
    assert L.ofx_flow_median(d, 4, None) == OFX_E_INVALID and b"item 3" in L.ofx_last_error()


def test_the_session_calls_refuse_a_null_session():
    from cuda_optical_flow_2_amd import lib

    L = lib.load()
    assert L.ofx_session_run_flow_dense_median(None, 9.0, 2, 0x10000000, 1 << 20, None) == OFX_E_INVALID and b"null session" in L.ofx_last_error()
    n = C.c_size_t()
    assert L.ofx_session_dense_median_scratch_bytes(None, C.byref(n)) == OFX_E_INVALID


def test_the_selection_networks_select_the_median_of_every_zero_one_input(tmp_path):
    """tests/median_net_check.cpp instantiates csrc/median_net.h on 64-bit words of 0-1 inputs: all 2^9 and 2^25 windows of each
    of a quad's four outputs, the other wires at 0 and at 1"""
    exe = tmp_path / "median_net_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "cuda_optical_flow_2_amd", "csrc"),
                    os.path.join(ROOT, "tests", "median_net_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(8 * (2 ** 9 + 2 ** 25))], r.stdout
