"""CPU: the stream pipeline's output stage (ofx_session_stream_compose / ofx_session_composed_of) is exported, declared in
include/ofx.h and bound in lib._SIGS; its timing kind is known on both sides."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ofx_session_stream_compose", "ofx_session_composed_of")


def _header():
    return open(os.path.join(ROOT, "include", "ofx.h")).read()


def test_compose_calls_are_exported_declared_and_bound():
    from cuda_optical_flow_2_amd import build, lib

    build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    declared = set(re.findall(r"\b(ofx_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    for name in NEW:
        assert name in exported, name
        assert name in declared, name
        assert name in lib._SIGS and name in lib.EXPORTS, name
    L = lib.load()
    assert L.ofx_abi_version() == 10
    # (no session: both refuse with OFX_E_INVALID instead of touching anything)
    assert L.ofx_session_stream_compose(None, 0, None, 0, 0) == 1
    assert L.ofx_session_composed_of(None, 1, None, None, None) == 1


def test_compose_timing_kind():
    from cuda_optical_flow_2_amd import engine

    kinds = dict(re.findall(r"#define (OFX_TIME_[A-Z_]+) (\d+)", _header()))
    assert kinds["OFX_TIME_COMPOSE"] == "8" and kinds["OFX_TIME_KINDS"] == "9"
    assert engine.Session.TIME_KINDS["compose"] == 8
    assert len(engine.Session.TIME_KINDS) == 9
