"""CPU: the sampled output stage's five calls (ofx_sample_arrows, ofx_advect_points, ofx_session_stream_arrows, _arrows_of,
_stream_tracks) are declared in include/ofx.h, exported by the library and bound in lib.py; the session calls refuse a NULL
session; the ABI version did not move.  No compute calls."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ofx_sample_arrows", "ofx_advect_points", "ofx_session_stream_arrows", "ofx_session_arrows_of", "ofx_session_stream_tracks"]


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


def test_session_calls_refuse_a_null_session():
    from cuda_optical_flow_2_amd import lib

    L = lib.load()
    assert L.ofx_session_stream_arrows(None, 0, 30, None, 0, 0) == 1
    assert b"null session" in L.ofx_last_error()
    assert L.ofx_session_arrows_of(None, 1, None, None, None) == 1
    assert L.ofx_session_stream_tracks(None, 0, None, None, 0, None, 0, 0) == 1
    assert b"null session" in L.ofx_last_error()


def test_abi_version_and_timing_kinds_did_not_move():
    from cuda_optical_flow_2_amd import engine, lib

    assert lib.load().ofx_abi_version() == 10
    text = open(os.path.join(ROOT, "include", "ofx.h")).read()
    assert re.search(r"#define\s+OFX_TIME_KINDS\s+9\b", text)
    assert len(engine.Session.TIME_KINDS) == 9


def test_arrow_grid():
    from cuda_optical_flow_2_amd import engine

    assert engine.arrow_grid(3840, 2160, 30) == (128, 17, 30)
    assert engine.arrow_grid(640, 480, 30) == (21, 23, 31)     # 640 = 30 * 21 + 10: a 31st, partial column
    assert engine.arrow_grid(64, 48, 64) == (1, 48, 64)
