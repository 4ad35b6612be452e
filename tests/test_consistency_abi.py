"""CPU: the forward-backward check's two calls (ofx_flow_consistency, ofx_flow_consistency_batch) are declared in include/ofx.h,
exported by the library and bound in lib.py; bad sizes, pitches, alignments, tolerances and batch arrays are refused with
OFX_E_INVALID before anything is enqueued; the ABI version and the timing kinds did not move.  No compute calls."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ofx_flow_consistency", "ofx_flow_consistency_batch"]
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
    # the bound argument lists are the header's: as many arguments, floats where it has floats
    for name in CALLS:
        args = re.search(name + r"\s*\(([^;]*)\)\s*;", text).group(1).split(",")
        assert len(args) == len(lib._SIGS[name]), name
        for decl, bound in zip(args, lib._SIGS[name]):
            assert (bound is C.c_float) == bool(re.match(r"float\s+\w", decl.strip())), (name, decl)
            assert (bound is C.c_int) == bool(re.match(r"int\s+\w", decl.strip())), (name, decl)


def test_python_surface_and_the_class_constants():
    from cuda_optical_flow_2_amd import engine

    for name in ("flow_consistency", "video_consistency"):
        assert callable(getattr(engine, name))
    text = open(os.path.join(ROOT, "include", "ofx.h")).read()
    for value, name in enumerate(("OFX_FB_CONSISTENT", "OFX_FB_INCONSISTENT", "OFX_FB_LEAVES", "OFX_FB_UNDEFINED")):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)\b", text).group(1)) == value


def test_the_stateless_call_refuses_bad_arguments_before_it_enqueues_anything():
    """The addresses are never dereferenced: every case below fails a check on the host."""
    from cuda_optical_flow_2_amd import lib

    L = lib.load()
    F, B, M, E, S = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000    # made-up, suitably aligned addresses
    w, h = 64, 8

    def call(fwd=F, bwd=B, w=w, h=h, scale=0.5, alpha=0.01, beta=0.5, mask=M, mp=64, err=E, stats=S):
        return L.ofx_flow_consistency(fwd, bwd, w, h, scale, alpha, beta, mask, mp, err, stats, None)

    assert call(fwd=None) == OFX_E_INVALID and call(bwd=None) == OFX_E_INVALID
    assert call(mask=None, err=None, stats=None) == OFX_E_INVALID       # nothing asked for
    assert call(w=0) == OFX_E_INVALID and call(h=0) == OFX_E_INVALID and call(w=-4) == OFX_E_INVALID and call(h=-1) == OFX_E_INVALID
    assert call(mp=63) == OFX_E_INVALID                                   # a pitch below the width
    assert b"pitch" in L.ofx_last_error()
    for kw in (dict(fwd=F + 4), dict(bwd=B + 4), dict(err=E + 2), dict(stats=S + 4)):
        assert call(**kw) == OFX_E_INVALID, kw
        assert b"aligned" in L.ofx_last_error(), kw
    assert call(w=1 << 14, h=1 << 14, mp=1 << 14) == OFX_E_INVALID      # 2^28 pixels
    assert call(w=1 << 16, h=1 << 16, mp=1 << 16) == OFX_E_INVALID      # (w * h does not fit an int)
    for bad in (NAN, -0.5, INF, -INF):
        assert call(alpha=bad) == OFX_E_INVALID, bad
        assert call(beta=bad) == OFX_E_INVALID, bad
    for bad in (NAN, INF, -INF):
        assert call(scale=bad) == OFX_E_INVALID, bad


def test_the_batch_call_refuses_bad_arguments_before_it_enqueues_anything():
    from cuda_optical_flow_2_amd import lib

    L = lib.load()
    vp = C.c_void_p

    def arr(base, n=17, hole=None, step=0x100000):
        return (vp * n)(*[None if i == hole else base + i * step for i in range(n)])

    F, B, M, E, S = arr(0x10000000), arr(0x20000000), arr(0x30000000), arr(0x40000000), arr(0x50000000)
    w, h = 64, 8

    def call(fwd=F, bwd=B, n=3, w=w, h=h, scale=0.5, alpha=0.01, beta=0.5, mask=M, mp=64, err=E, stats=S):
        return L.ofx_flow_consistency_batch(fwd, bwd, n, w, h, scale, alpha, beta, mask, mp, err, stats, None)

    assert call(n=0) == OFX_E_INVALID and call(n=17) == OFX_E_INVALID and call(n=-1) == OFX_E_INVALID
    assert call(fwd=None) == OFX_E_INVALID and call(bwd=None) == OFX_E_INVALID
    assert call(mask=None, err=None, stats=None) == OFX_E_INVALID       # at least one output array
    for kw in ("fwd", "bwd", "mask", "err", "stats"):                   # a NULL entry in a non-NULL array
        assert call(**{kw: arr(0x60000000, hole=2)}) == OFX_E_INVALID, kw
    assert call(mp=63) == OFX_E_INVALID
    assert b"pitch" in L.ofx_last_error()
    for kw, off in (("fwd", 4), ("bwd", 4), ("err", 2), ("stats", 4)):  # one misaligned entry, not the first
        a = arr(0x60000000)
        a[1] = 0x60000000 + 0x100000 + off
        assert call(**{kw: a}) == OFX_E_INVALID, kw
        assert b"aligned" in L.ofx_last_error(), kw
    assert call(w=1 << 14, h=1 << 14, mp=1 << 14) == OFX_E_INVALID
    assert call(alpha=NAN) == OFX_E_INVALID and call(alpha=-1.0) == OFX_E_INVALID
    assert call(beta=NAN) == OFX_E_INVALID and call(beta=-1.0) == OFX_E_INVALID
    assert call(scale=INF) == OFX_E_INVALID and call(scale=NAN) == OFX_E_INVALID


def test_abi_version_and_timing_kinds_did_not_move():
    from cuda_optical_flow_2_amd import engine, lib

    assert lib.load().ofx_abi_version() == 10
    text = open(os.path.join(ROOT, "include", "ofx.h")).read()
    assert re.search(r"#define\s+OFX_TIME_KINDS\s+9\b", text)
    assert len(engine.Session.TIME_KINDS) == 9
