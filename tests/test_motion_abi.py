"""CPU: the motion-compensation stage's three calls (ofx_motion_compensate, ofx_session_stream_motion, ofx_session_motion_of) are
declared in include/ofx.h, exported by the library and bound in lib.py; a NULL session and bad sizes, pitches and alignments
are refused with the documented codes before anything is enqueued; the ABI version and the timing kinds did not move.  No
compute calls.  (What ofx_session_stream_motion refuses on a live session -- alignment, pitch, stride, n_slots, state,
sharded -- needs a device: tests/test_gpu_motion.py::test_refusals.)"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ofx_motion_compensate", "ofx_session_stream_motion", "ofx_session_motion_of"]
OFX_E_INVALID = 1


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


def test_python_surface():
    from cuda_optical_flow_2_amd import engine

    for name in ("motion_compensate", "video_motion"):
        assert callable(getattr(engine, name))
    for name in ("stream_motion", "motion_of"):
        assert callable(getattr(engine.Session, name))
    text = open(os.path.join(ROOT, "include", "ofx.h")).read()
    scale = float(re.search(r"#define\s+OFX_ITER_SCALE\s+([0-9.]+)f", text).group(1))
    assert engine.ITER_SCALE == scale


def test_session_calls_refuse_a_null_session():
    from cuda_optical_flow_2_amd import lib

    L = lib.load()
    assert L.ofx_session_stream_motion(None, 0, 0.5, None, 0, 0, 0, None) == OFX_E_INVALID
    assert b"null session" in L.ofx_last_error()
    assert L.ofx_session_stream_motion(None, 0, 0.5, 4096, 64, 4096, 4, 8192) == OFX_E_INVALID
    assert L.ofx_session_motion_of(None, 1, None, None, None) == OFX_E_INVALID
    assert b"null session" in L.ofx_last_error()


def test_the_stateless_call_refuses_bad_arguments_before_it_enqueues_anything():
    """The addresses are never dereferenced: every case below fails a check on the host."""
    from cuda_optical_flow_2_amd import lib

    L = lib.load()
    P, N, F, D, S = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000    # made-up, suitably aligned addresses
    w, h = 64, 8

    def call(prev=P, pp=64, nxt=N, np_=64, w=w, h=h, flow=F, uv=None, dst=D, dp=64, stats=S):
        return L.ofx_motion_compensate(prev, pp, nxt, np_, w, h, flow, uv, 0.5, dst, dp, stats, None)

    assert call(prev=None) == OFX_E_INVALID and call(nxt=None) == OFX_E_INVALID and call(flow=None) == OFX_E_INVALID
    assert call(dst=None, stats=None) == OFX_E_INVALID                 # nothing asked for
    assert call(w=0) == OFX_E_INVALID and call(h=0) == OFX_E_INVALID and call(w=-4) == OFX_E_INVALID
    assert call(pp=63) == OFX_E_INVALID and call(np_=60) == OFX_E_INVALID and call(dp=63) == OFX_E_INVALID   # a pitch below the width
    assert b"pitch" in L.ofx_last_error()
    assert call(flow=F + 4) == OFX_E_INVALID                            # flow: 8-byte aligned
    assert call(stats=S + 4) == OFX_E_INVALID                           # stats: 8-byte aligned
    assert b"aligned" in L.ofx_last_error()
    assert call(uv=0x60002) == OFX_E_INVALID
    assert call(pp=1 << 20, h=1 << 11) == OFX_E_INVALID                 # a plane of 2^31 bytes


def test_abi_version_and_timing_kinds_did_not_move():
    from cuda_optical_flow_2_amd import engine, lib

    assert lib.load().ofx_abi_version() == 10
    text = open(os.path.join(ROOT, "include", "ofx.h")).read()
    assert re.search(r"#define\s+OFX_TIME_KINDS\s+9\b", text)
    assert len(engine.Session.TIME_KINDS) == 9
