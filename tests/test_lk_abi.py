"""CPU: the descriptors of the stateless launch ABI -- ofx_lk_desc, ofx_shift_desc, ofx_warp_desc and the ofx_geom inside them --
have, compiled from include/ofx.h as C and as C++, the size and the field offsets of their ctypes twins in lib.py (LkDesc, ShiftDesc,
WarpDesc, Geom).  A few lines are compiled and run on the host; no compute calls."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = [("ofx_geom", "Geom"), ("ofx_lk_desc", "LkDesc"), ("ofx_shift_desc", "ShiftDesc"), ("ofx_warp_desc", "WarpDesc")]


def _twin(name):
    from cuda_optical_flow_2_amd import lib

    return getattr(lib, name)


@pytest.mark.parametrize("cc,flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_the_descriptors_have_the_layout_of_their_ctypes_twins(tmp_path, cc, flags):
    lines = []
    for cname, pyname in STRUCTS:
        fields = [f[0] for f in _twin(pyname)._fields_]
        lines.append(f'printf("{cname} %zu", sizeof({cname}));')
        lines += [f'printf(" %zu", offsetof({cname}, {f}));' for f in fields]
        lines.append('printf("\\n");')
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "ofx.h"\nint main(void){' + "".join(lines) + "return 0;}\n"
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = tmp_path / "t"
    subprocess.run([cc, "-Wall", "-Werror"] + flags + [str(c), "-I", os.path.join(ROOT, "include"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(STRUCTS)
    for line, (cname, pyname) in zip(out, STRUCTS):
        words = line.split()
        t = _twin(pyname)
        assert words[0] == cname
        assert int(words[1]) == C.sizeof(t), f"sizeof({cname}) = {words[1]}, lib.{pyname} has {C.sizeof(t)}"
        got = [int(v) for v in words[2:]]
        want = [getattr(t, f[0]).offset for f in t._fields_]
        assert got == want, f"{cname}: offsets {got}, lib.{pyname} has {want} for {[f[0] for f in t._fields_]}"


def test_the_twins_name_every_field_of_the_header():
    """the other direction: a field added to a struct of the header must appear in its twin (the offsets above cannot see a missing
    last field that fits into the tail padding)"""
    import re

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofx.h")).read(), flags=re.S)
    for cname, pyname in STRUCTS:
        body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", text, flags=re.S).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            first, *rest = decl.split(",")
            names.append(re.findall(r"[A-Za-z_0-9]+", first)[-1])
            names += [re.findall(r"[A-Za-z_0-9]+", r)[-1] for r in rest]
        assert names == [f[0] for f in _twin(pyname)._fields_], (cname, names)


def test_engine_uses_the_shared_warp_descriptor():
    from cuda_optical_flow_2_amd import engine, lib
    import inspect

    assert "class WarpDesc" not in inspect.getsource(engine.warp_u8) and "WarpDesc" in inspect.getsource(engine.warp_u8)
    assert lib._SIGS["ofx_lk_levels"][0] == C.c_void_p and lib._SIGS["ofx_shift_levels"][0] == C.c_void_p and lib._SIGS["ofx_warp_levels"][0] == C.c_void_p


def test_the_stateless_calls_refuse_bad_descriptors_on_the_host():
    """The refusals of tests/lk_abi_cases.py on made-up addresses: each fails a check before anything is enqueued, so nothing is
    dereferenced and no device is needed.  (tests/test_gpu_lk_abi.py repeats them on real allocations.)"""
    from cuda_optical_flow_2_amd import build, lib
    import lk_abi_cases as K

    build.build()
    L = lib.load()
    cases = K.refusals(lib, 0x10000000)
    assert len(cases) >= 40
    for what, code, word, call in cases:
        rc = call(L)
        msg = L.ofx_last_error()
        assert rc == code, (what, rc, msg)
        assert msg and word in msg, (what, msg)


def test_the_launches_select_the_kernels_the_cases_are_about(tmp_path):
    """tools/lk_plan_main.cpp (csrc/lk_plan.h) on the launches of tests/test_gpu_lk_abi.py: accumulate in compat_cpu stays in the level
    kernel (lk_level_kernel, MODE 0: its MAY_ACC path), the lk_float variants run ITER 1 / 2 / 3 of the buffer march and ITER 4 on the
    row windows, and OFX_ITER_DMA=1 -- the child process -- turns each of those into its deep-fetch form."""
    import lk_abi_cases as K
    import lk_plan_ref as ref
    from test_lk_plan import compile_tool, item, line_of, parse

    exe = compile_tool(tmp_path, "lk_plan_main")
    lines, wants = [], []

    def add(mode, win, items, acc, wout, want, dma=None):
        items = [dict(a, accumulate=acc, warp_out=wout) for a in items]
        lines.append(line_of("levels", items, dict(ref.ENV, OFX_ITER_DMA=dma), mode=mode, window=win))
        wants.append(want)

    def one(w, h, g, rows=None):
        row0, n, y0, y1, f0 = rows if rows else (0, h, 0, h, 0)
        return item(w, h, out=(y0, y1), rows=(row0, row0 + n), pitch=K.pitch_of(g.pitch, w), flow_row0=f0)

    for acc in K.ACC_COMPAT:
        add(0, acc.win, [one(w, h, g, rows) for (w, h, rows, g) in acc.items], 1, 0, dict(family="levels", mode=0, fast=0, sums=0, iter=0, deep=0, many=0))
    for mi, mode in enumerate(K.ITER_MODES):
        for dma in (None, 1):
            for si, (w, h, win) in enumerate(K.ITER_SHAPES):
                for vi, (variant, aw, it) in enumerate(zip(K.ITER_VARIANTS, ((1, 0), (1, 1), (0, 1)), (1, 2, 3))):
                    add(1 + mi, win, [one(w, h, K.geo(si + vi))], *aw, dict(family="iter", mode=1, fast=mi, sums=0, iter=it, deep=int(dma == 1), many=0), dma)
            for c in (K.ROWS_NO_MISS, K.ROWS_MISS):
                add(1 + mi, c["win"], [one(c["w"], c["h"], K.geo(4), c["rows"])], 1, 1, dict(family="iter", mode=1, fast=mi, sums=0, iter=4, deep=int(dma == 1), many=0), dma)
    for (w, h, win, _, warp, g) in K.ITER_UV:
        add(1, win, [one(w, h, g)], 1, int(warp), dict(family="iter", mode=1, fast=0, sums=0, iter=2 if warp else 1, deep=0, many=0))
    text = subprocess.run([exe], input="".join(l + "\n" for l in lines), text=True, check=True, stdout=subprocess.PIPE).stdout
    got = parse(text, len(lines))
    assert len(got) == len(lines) > 150
    for line, g, want in zip(lines, got, wants):
        assert not isinstance(g, ref.Rejected), (line, g)
        assert g["variant"] == want, (line, g["variant"])
