"""CPU: the stream pipeline's colour front end (ofx_frontend_1ch, ofx_session_stream_frontend, ofx_session_stream_submit_3ch,
ofx_session_stream_submit_frames_3ch) is exported, declared in include/ofx.h and bound in lib._SIGS; calls without a session
refuse with OFX_E_INVALID, and the ABI version stays 10."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofx_frontend_1ch", "ofx_session_stream_frontend", "ofx_session_stream_submit_3ch", "ofx_session_stream_submit_frames_3ch")


def _header():
    return open(os.path.join(ROOT, "include", "ofx.h")).read()


def test_frontend_calls_are_exported_declared_and_bound():
    from cuda_optical_flow_2_amd import build, lib

    build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    declared = set(re.findall(r"\b(ofx_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    for name in NEW:
        assert name in exported, name
        assert name in declared, name
        assert name in lib._SIGS and name in lib.EXPORTS, name
    assert lib.load().ofx_abi_version() == 10


def test_frontend_calls_without_a_session_are_invalid():
    from cuda_optical_flow_2_amd import lib

    L = lib.load()
    done = C.c_int(7)
    assert L.ofx_session_stream_frontend(None, 2, 9, 2.0, 10.0, 0) == 1
    assert L.ofx_session_stream_frontend(None, 0, 0, 0.0, 0.0, 0) == 1
    assert L.ofx_session_stream_submit_3ch(None, None, 0, None, C.byref(done)) == 1
    frames = (C.c_void_p * 1)(None)
    assert L.ofx_session_stream_submit_frames_3ch(None, frames, None, 0, 1, None, C.byref(done)) == 1
    assert L.ofx_frontend_1ch(None, None, 0, None, None, 0, 1, 4, 4, None, 1, 9, 2.0, 10.0, None) == 1
    assert L.ofx_abi_version() == 10


def test_frontend_constants_and_refusals_before_any_launch():
    """The mode / flag values both sides use; an unsupported window is refused (OFX_E_UNSUPPORTED) while the tables are built,
    before anything reaches a device."""
    from cuda_optical_flow_2_amd import engine, lib

    d = dict(re.findall(r"#define (OFX_FRONTEND_[A-Z_]+) (\d+)", _header()))
    assert (d["OFX_FRONTEND_OFF"], d["OFX_FRONTEND_GREY"], d["OFX_FRONTEND_BILATERAL"], d["OFX_FRONTEND_BILATERAL_FAST"]) == ("0", "1", "2", "3")
    assert (d["OFX_FRONTEND_FLAG_FAST"], d["OFX_FRONTEND_FLAG_FIRST_GREY"]) == ("1", "2")
    assert engine.Session.FRONTEND_MODES == {"off": 0, "grey": 1, "bilateral": 2}
    L = lib.load()
    src = (C.c_void_p * 1)(4096)   # (never dereferenced: the call is refused first)
    dst = (C.c_void_p * 1)(8192)
    for window in (1, 4, 15, 19):
        assert L.ofx_frontend_1ch(src, None, 12, dst, None, 4, 1, 4, 4, None, 2, window, 2.0, 10.0, None) == 3, window
    assert L.ofx_frontend_1ch(src, None, 12, dst, None, 4, 17, 4, 4, None, 2, 9, 2.0, 10.0, None) == 1   # more than 16 frames
    assert L.ofx_frontend_1ch(src, None, 12, dst, None, 4, 1, 4, 4, None, 2, 9, 0.0, 10.0, None) == 1    # sigma_s <= 0
