"""CPU: ofx_fit_motion, ofx_fit_motion_work_bytes, ofx_motion_compose and ofx_motion_invert are declared in include/ofx.h, exported
by the library and bound in lib.py; the header compiles as C and as C++ and ofx_fit_desc / ofx_fit_params have the layouts of their
ctypes twins; the ABI version did not move; the call refuses bad arguments with OFX_E_INVALID and a message that names the item
and the argument, before anything is enqueued; the two host helpers agree with NumPy by the bits.  No compute on a device."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import fit_motion_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFX_E_INVALID = 1
NAMES = ("ofx_fit_motion", "ofx_fit_motion_work_bytes", "ofx_motion_compose", "ofx_motion_invert")


def test_declared_exported_and_bound():
    from cuda_optical_flow_2_amd import build, lib

    build.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ofx_[a-z0-9_]+)\s*\(", text))
    nm = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    L = lib.load()
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/ofx.h"
        assert name in exported, f"{name} is not exported by the library"
        assert name in lib.EXPORTS and name in lib._SIGS, f"{name} is not in lib.EXPORTS / lib._SIGS"
        assert getattr(L, name).argtypes == lib._SIGS[name]
    vp = C.c_void_p
    assert lib._SIGS["ofx_fit_motion"] == [C.POINTER(lib.FitDesc), C.c_int, C.POINTER(lib.FitParams), vp]
    assert lib._SIGS["ofx_fit_motion_work_bytes"] == [C.POINTER(lib.FitParams)] and L.ofx_fit_motion_work_bytes.restype == C.c_size_t
    assert lib._SIGS["ofx_motion_compose"] == [vp, vp, vp] and lib._SIGS["ofx_motion_invert"] == [vp, vp]
    assert "fit_motion.hip" in build.SOURCES
    for word, value in (("OFX_MOTION_TRANSLATION", 0), ("OFX_MOTION_SIMILARITY", 1), ("OFX_MOTION_AFFINE", 2), ("OFX_FIT_OK", 0), ("OFX_FIT_FEW", 1),
                        ("OFX_FIT_DEGENERATE", 2)):
        assert re.search(rf"#define\s+{word}\s+{value}\b", text)


def test_python_surface():
    from cuda_optical_flow_2_amd import engine

    p = inspect.signature(engine.fit_motion).parameters
    assert list(p) == ["p", "q", "size", "status", "pair", "model", "hypotheses", "thr", "refits", "seed", "return_inliers"]
    assert [p[k].default for k in list(p)[3:]] == [None, 0, "similarity", 256, 1.0, 2, 0, False]
    p = inspect.signature(engine.video_camera_motion).parameters
    assert list(p) == ["frames", "model", "levels", "window", "cell", "reseed", "hypotheses", "thr", "refits", "seed", "max_iters", "eps", "min_lambda",
                       "max_sad"]
    assert [p[k].default for k in list(p)[1:]] == ["similarity", 3, 9, 16, 16, 256, 1.0, 2, 0, 10, 1 / 32, 0.0, 0]
    assert list(inspect.signature(engine.motion_compose).parameters) == ["m2", "m1"]
    assert list(inspect.signature(engine.motion_invert).parameters) == ["m"]
    assert list(inspect.signature(engine.smooth_path).parameters) == ["models", "radius"]
    assert engine.MOTION_MODELS == {"translation": 0, "similarity": 1, "affine": 2}
    assert (engine.FIT_OK, engine.FIT_FEW, engine.FIT_DEGENERATE) == (0, 1, 2)


@pytest.mark.parametrize("cc,flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_the_header_compiles_and_the_structs_have_the_bound_layouts(tmp_path, cc, flags):
    from cuda_optical_flow_2_amd import lib

    desc = [f[0] for f in lib.FitDesc._fields_]
    prm = [f[0] for f in lib.FitParams._fields_]
    assert desc == ["d_p", "d_q", "d_status", "n", "pair", "w", "h", "d_model", "d_info", "d_inlier", "d_work"]
    assert prm == ["model", "hypotheses", "thr_q", "refits", "seed"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ofx.h"\n'
           'int main(void){ofx_fit_desc c; ofx_fit_params p; (void)c; (void)p;\n'
           'printf("%zu %zu %zu", sizeof(ofx_fit_desc), sizeof(ofx_fit_params), sizeof(ofx_params));\n'
           + "".join(f'printf(" %zu", offsetof(ofx_fit_desc, {f}));\n' for f in desc)
           + "".join(f'printf(" %zu", offsetof(ofx_fit_params, {f}));\n' for f in prm) + 'printf("\\n"); return 0;}\n')
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = tmp_path / "t"
    subprocess.run([cc, "-Wall", "-Werror"] + flags + [str(c), "-I", os.path.join(ROOT, "include"), "-o", str(exe)], check=True)
    s_desc, s_prm, params, *offs = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert s_desc == C.sizeof(lib.FitDesc) and s_prm == C.sizeof(lib.FitParams)
    assert offs == [getattr(lib.FitDesc, f).offset for f in desc] + [getattr(lib.FitParams, f).offset for f in prm]
    assert params == C.sizeof(lib.Params), "sizeof(ofx_params) moved"


def test_abi_version_did_not_move():
    from cuda_optical_flow_2_amd import lib

    assert lib.load().ofx_abi_version() == 10
    text = open(os.path.join(ROOT, "include", "ofx.h")).read()
    assert re.search(r"#define\s+OFX_STREAM_MAX_BATCH\s+16\b", text)
    assert C.sizeof(lib.Params) == 352


def test_work_bytes_is_host_arithmetic():
    from cuda_optical_flow_2_amd import lib

    L = lib.load()
    for H in (1, 7, 256, 4096):
        nbytes = L.ofx_fit_motion_work_bytes(C.byref(lib.FitParams(1, H, 32, 2, 0)))
        assert nbytes >= 56 * H and nbytes % 8 == 0 and nbytes <= 1 << 20
    assert L.ofx_fit_motion_work_bytes(None) == 0
    assert L.ofx_fit_motion_work_bytes(C.byref(lib.FitParams(1, 0, 32, 2, 0))) == 0
    assert L.ofx_fit_motion_work_bytes(C.byref(lib.FitParams(1, 4097, 32, 2, 0))) == 0


def test_fit_motion_refuses_bad_arguments_before_it_enqueues_anything():
    """The addresses are never dereferenced: every case below fails a check on the host."""
    from cuda_optical_flow_2_amd import lib

    L = lib.load()
    P, Q, ST, MO, IN, MA, WK = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000, 0x70000000   # made-up addresses

    def call(n_items=2, bad=1, items="ok", prm="ok", model=1, hypotheses=256, thr_q=32, refits=2, seed=0, **kw):
        descs = (lib.FitDesc * max(n_items, 1))()
        for i in range(max(n_items, 1)):
            f = dict(d_p=P, d_q=Q, d_status=ST, n=100 + i, pair=3, w=640, h=480, d_model=MO + 64 * i, d_info=IN + 32 * i, d_inlier=MA, d_work=WK + (i << 20))
            if i == min(bad, max(n_items, 1) - 1):
                f.update(kw)
            descs[i] = lib.FitDesc(**f)
        p = lib.FitParams(model, hypotheses, thr_q, refits, seed)
        rc = L.ofx_fit_motion(descs if items == "ok" else None, n_items, C.byref(p) if prm == "ok" else None, None)
        return rc, L.ofx_last_error()

    def refused(word, item=None, **kw):
        rc, msg = call(**kw)
        assert rc == OFX_E_INVALID, (kw, rc)
        assert msg and word in msg, (kw, msg)
        if item is not None:
            assert b"item %d" % item in msg, (kw, msg)

    refused(b"null", items=None)
    refused(b"null", prm=None)
    for name in ("d_p", "d_q", "d_model", "d_info", "d_work"):
        refused(b"null", item=1, **{name: None})
        refused(name.encode(), item=0, bad=0, **{name: None})
    for n_items in (0, -1, 17, 1 << 20):
        refused(b"n_items", n_items=n_items)
    for model in (-1, 3, 100):
        refused(b"model", model=model)
    for H in (0, -5, 4097, 1 << 30):
        refused(b"hypotheses", hypotheses=H)
    for thr_q in (-1, (1 << 15) + 1, 1 << 30):
        refused(b"thr_q", thr_q=thr_q)
    for refits in (-1, 4, 99):
        refused(b"refits", refits=refits)
    for n in (0, -1, (1 << 20) + 1):
        refused(b"n =", item=1, n=n)
    for kw in (dict(w=0), dict(h=0), dict(w=-3), dict(w=(1 << 16) + 1), dict(h=(1 << 16) + 1)):
        refused(b"size", item=1, **kw)
    for kw in (dict(d_p=P + 4), dict(d_q=Q + 4), dict(d_p=P + 1), dict(d_model=MO + 4), dict(d_work=WK + 4)):
        refused(b"8-byte", item=1, **kw)
    for kw in (dict(d_info=IN + 2), dict(d_info=IN + 1), dict(d_status=ST + 2)):
        refused(b"4-byte", item=1, **kw)
    # what is allowed passes every check up to a refused last one: the limits of each range, no status, no mask, an odd mask address
    for kw in (dict(model=0, hypotheses=1, thr_q=0, refits=0, seed=0xFFFFFFFF, n_items=1, bad=0), dict(model=2, hypotheses=4096, thr_q=1 << 15, refits=3, n_items=16, bad=15),
               dict(d_status=None, d_inlier=None), dict(d_inlier=MA + 1, pair=-4, n=1 << 20, w=1 << 16, h=1), dict(n=1, w=1, h=1 << 16)):
        refused(b"d_info", d_info=IN + 2, **kw)


def test_compose_and_invert_agree_with_numpy_by_the_bits():
    from cuda_optical_flow_2_amd import engine, lib

    rng = np.random.default_rng(11)
    bits = lambda a: np.asarray(a, np.float64).view(np.int64).tolist()
    cases = [np.array(R.IDENTITY), np.array([1.0, -0.0, 4.0, 0.0, 1.0, -3.0]), np.array([1.03, -0.02, 3.3, 0.02, 1.03, -1.7]),
             np.array([1e-100, 0.0, 1e100, 0.0, 1e-100, -1e100]), np.array([16.0, -16.0, 1048576.0, 15.999, 16.0, -1048576.0])]
    cases += [rng.normal(0.0, 1.0, 6) * 10.0 ** rng.integers(-3, 4, 6) for _ in range(40)]
    for i, a in enumerate(cases):
        for b in cases[::3] + [cases[(i + 1) % len(cases)]]:
            assert bits(engine.motion_compose(a, b)) == bits(R.compose(a, b)), (a, b)
        want = R.invert(a)
        assert want is not None and bits(engine.motion_invert(a)) == bits(want), a
    out = np.zeros(6)
    L = lib.load()
    for m in ([1, 2, 0, 2, 4, 0], [0, 0, 0, 0, 0, 0], [np.inf, 0, 0, 0, 1, 0], [np.nan, 0, 0, 0, 1, 0], [1e200, 0, 0, 0, 1e200, 0]):
        a = np.array(m, np.float64)
        assert R.invert(a) is None
        assert L.ofx_motion_invert(a.ctypes.data, out.ctypes.data) == OFX_E_INVALID and b"determinant" in L.ofx_last_error()
        with pytest.raises(lib.OfxError):
            engine.motion_invert(a)
    assert L.ofx_motion_invert(None, out.ctypes.data) == OFX_E_INVALID and L.ofx_motion_compose(out.ctypes.data, None, out.ctypes.data) == OFX_E_INVALID
    assert not out.any(), "a refused call writes nothing"
    # out may be an input
    a, b = cases[2].copy(), cases[4].copy()
    want = R.compose(a, b)
    assert L.ofx_motion_compose(a.ctypes.data, b.ctypes.data, a.ctypes.data) == 0 and bits(a) == bits(want)


def test_smooth_path_is_the_clipped_mean_in_index_order():
    from cuda_optical_flow_2_amd import engine

    rng = np.random.default_rng(3)
    m = rng.normal(0.0, 1.0, (9, 6))
    assert engine.smooth_path(m, 0).view(np.int64).tolist() == m.view(np.int64).tolist()
    for radius in (1, 3, 20):
        got = engine.smooth_path(m, radius)
        for f in range(9):
            g0, g1 = max(f - radius, 0), min(f + radius, 8)
            for e in range(6):
                s = np.float64(0.0)
                for g in range(g0, g1 + 1):
                    s = s + m[g, e]
                assert got[f, e] == s / np.float64(g1 - g0 + 1)
