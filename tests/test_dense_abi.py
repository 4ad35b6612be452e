"""CPU: the coarse-to-fine calls (ofx_flow_prolong, ofx_session_run_flow_dense) are declared in include/ofx.h, exported by the
library and bound in lib.py; the header compiles as C and as C++ and ofx_prolong_desc has the size of its ctypes twin; ofx_params,
the ABI version and the timing kinds did not move; ofx_flow_prolong refuses bad descriptors with OFX_E_INVALID and a message before
anything is enqueued.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ofx_flow_prolong", "ofx_session_run_flow_dense"]
OFX_E_INVALID = 1
OFX_MAX_LEVELS = 12
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
    assert lib._SIGS["ofx_flow_prolong"] == [C.POINTER(lib.ProlongDesc), C.c_int, C.c_void_p]
    assert lib._SIGS["ofx_session_run_flow_dense"] == [C.c_void_p, C.c_float, C.c_void_p]


def test_python_surface():
    from cuda_optical_flow_2_amd import engine
    import inspect

    assert callable(engine.Session.run_flow_dense)
    for name, first in (("flow_pair_dense", ["prev1", "next1", "levels", "window", "iters", "min_det", "max_px"]),
                        ("video_displacement_dense", ["frames", "levels", "window", "iters", "min_det", "max_px", "level", "out"]),
                        ("video_interpolate_dense", ["frames", "levels", "window", "factor", "iters", "min_det", "max_px"])):
        sig = inspect.signature(getattr(engine, name))
        assert list(sig.parameters)[:len(first)] == first, (name, list(sig.parameters))
        assert sig.parameters["iters"].default == 3 and sig.parameters["min_det"].default == 1.0 and sig.parameters["max_px"].default is None
    assert inspect.signature(engine.Session.run_flow_dense).parameters["max_px"].default is None


@pytest.mark.parametrize("cc,flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_the_header_compiles_and_the_struct_has_the_bound_size(tmp_path, cc, flags):
    from cuda_optical_flow_2_amd import lib

    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ofx.h"\n'
           'int main(void){ofx_prolong_desc d; (void)d; printf("%zu %zu %zu %zu %zu\\n", sizeof(ofx_prolong_desc), sizeof(ofx_params), '
           'offsetof(ofx_prolong_desc, d_fine), offsetof(ofx_prolong_desc, d_src), offsetof(ofx_prolong_desc, dst_pitch));'
           'return 0;}\n')
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = tmp_path / "t"
    subprocess.run([cc, "-Wall", "-Werror"] + flags + [str(c), "-I", os.path.join(ROOT, "include"), "-o", str(exe)], check=True)
    size, params, o_fine, o_src, o_dp = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == C.sizeof(lib.ProlongDesc)
    assert (o_fine, o_src, o_dp) == (lib.ProlongDesc.d_fine.offset, lib.ProlongDesc.d_src.offset, lib.ProlongDesc.dst_pitch.offset)
    assert params == C.sizeof(lib.Params), "sizeof(ofx_params) moved"


def test_abi_version_params_and_timing_kinds_did_not_move():
    from cuda_optical_flow_2_amd import engine, lib

    assert lib.load().ofx_abi_version() == 10
    text = open(os.path.join(ROOT, "include", "ofx.h")).read()
    assert re.search(r"#define\s+OFX_TIME_KINDS\s+9\b", text)
    assert len(engine.Session.TIME_KINDS) == 9
    # ofx_params as the parent commit had it: 6 ints, the sharding block (1 + 6 * OFX_MAX_LEVELS ints), then iters .. deep_fetch
    assert C.sizeof(lib.Params) == 4 * (6 + 1 + 6 * OFX_MAX_LEVELS + 5 + 1 + 3) == 352
    assert [f[0] for f in lib.Params._fields_][-9:] == ["iters", "local_corner", "patch_size", "stream_batch", "borrow_frames", "min_det",
                                                       "stream_two_stage", "frames_partial", "deep_fetch"]


def test_prolong_refuses_bad_descriptors_before_it_enqueues_anything():
    """The addresses are never dereferenced: every case below fails a check on the host."""
    from cuda_optical_flow_2_amd import lib

    L = lib.load()
    CO, FI, SRC, DST = 0x10000000, 0x20000000, 0x30000000, 0x40000000    # made-up, suitably aligned addresses

    def desc(coarse=CO, wc=20, hc=6, fine=FI, w=40, h=12, scale=0.5, max_px=9.0, src=SRC, sp=64, dst=DST, dp=64):
        return lib.ProlongDesc(coarse, wc, hc, fine, w, h, scale, max_px, src, sp, dst, dp)

    def refused(word, n=1, **kw):
        d = (lib.ProlongDesc * OFX_MAX_LEVELS)(*[desc() for _ in range(OFX_MAX_LEVELS)])
        d[max(min(n, OFX_MAX_LEVELS), 1) - 1] = desc(**kw)          # the bad one is the last of the launch
        rc = L.ofx_flow_prolong(d, n, None)
        msg = L.ofx_last_error()
        assert rc == OFX_E_INVALID, (kw, n, rc)
        assert msg and word in msg, (kw, n, msg)

    for n in (1, 3):
        for kw in (dict(w=39), dict(w=42), dict(h=11), dict(h=14), dict(w=41, h=10), dict(wc=0), dict(hc=-1)):   # sizes that are no 2x (+1)
            refused(b"size", n, **kw)
        for bad in (-1.0, NAN, INF, -INF, -1e-30):
            refused(b"max_px", n, max_px=bad)
        for kw in (dict(sp=39), dict(dp=39), dict(sp=0), dict(dp=-64)):
            refused(b"pitch", n, **kw)
        for kw in (dict(coarse=CO + 4), dict(fine=FI + 4), dict(fine=FI + 2)):
            refused(b"aligned", n, **kw)
        refused(b"d_src and d_dst", n, dst=None)
        refused(b"d_src and d_dst", n, src=None)
        # d_dst inside d_src's (h - 1) * pitch + w bytes, from either side; the byte behind the plane's last pixel is free
        for dst in (SRC, SRC + 11 * 64 + 39, SRC - 11 * 64 - 39, SRC + 4):
            refused(b"overlaps", n, dst=dst)
        refused(b"overlaps", n, fine=CO + 8)
        for kw in (dict(coarse=None), dict(fine=None)):
            refused(b"null", n, **kw)
    for n in (0, -1, OFX_MAX_LEVELS + 1, 1 << 20):
        refused(b"n = ", n)
    assert L.ofx_flow_prolong(None, 1, None) == OFX_E_INVALID and b"null" in L.ofx_last_error()
    # the odd sizes and a flow-only descriptor pass the checks of a descriptor that comes BEFORE a refused one
    d = (lib.ProlongDesc * 3)(desc(w=41, h=13, sp=41, dp=41), desc(src=None, dst=None, sp=0, dp=0), desc(max_px=-1.0))
    assert L.ofx_flow_prolong(d, 3, None) == OFX_E_INVALID and b"level 2" in L.ofx_last_error()


def test_the_session_call_refuses_a_null_session():
    from cuda_optical_flow_2_amd import lib

    L = lib.load()
    assert L.ofx_session_run_flow_dense(None, 9.0, None) == OFX_E_INVALID and b"null session" in L.ofx_last_error()
