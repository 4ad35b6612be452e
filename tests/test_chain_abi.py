"""CPU: ofx_displacement_chain is declared in include/ofx.h, exported by the library and bound in lib.py; the header compiles as C and
as C++ and ofx_chain_desc has the layout of its ctypes twin; nothing that existed moved; the Python surface; the call refuses bad
arguments with OFX_E_INVALID and a message that names the call, the item and, for a link, the link, before anything is enqueued.
No compute."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFX_E_INVALID = 1
NAME = "ofx_displacement_chain"


def test_declared_exported_and_bound():
    from cuda_optical_flow_2_amd import build, engine, lib

    build.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ofx_[a-z0-9_]+)\s*\(", text))
    nm = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    L = lib.load()
    assert NAME in declared, f"{NAME} is not declared in include/ofx.h"
    assert NAME in exported, f"{NAME} is not exported by the library"
    assert NAME in lib.EXPORTS and NAME in lib._SIGS, f"{NAME} is not in lib.EXPORTS / lib._SIGS"
    assert getattr(L, NAME).argtypes == lib._SIGS[NAME] == [C.POINTER(lib.ChainDesc), C.c_int, C.c_void_p]
    assert re.search(r"int\s+ofx_displacement_chain\(const ofx_chain_desc \*items, int n, void \*stream\);", text)
    assert "chain.hip" in build.SOURCES
    assert re.search(r"#define\s+OFX_CHAIN_MAX_LINKS\s+4\b", text)
    assert lib.OFX_CHAIN_MAX_LINKS == 4 == engine.CHAIN_MAX_LINKS
    for name, value in (("OK", 0), ("LEAVES", 2), ("UNDEFINED", 3)):
        assert re.search(rf"#define\s+OFX_CHAIN_{name}\s+{value}\b", text)
    assert re.search(r"#define\s+OFX_FB_LEAVES\s+2\b", text) and re.search(r"#define\s+OFX_FB_UNDEFINED\s+3\b", text)
    assert re.search(r"#define\s+OFX_TEMPORAL_MAX_NEIGHBOURS\s+4\b", text), "the filter's reach stays where it was"


def test_python_surface():
    from cuda_optical_flow_2_amd import engine

    p = inspect.signature(engine.displacement_chain).parameters
    assert list(p) == ["links", "return_mask", "return_stats"] and [p[k].default for k in list(p)[1:]] == [False, False]
    assert list(inspect.signature(engine.chain_ring).parameters) == ["ring", "span"]
    p = inspect.signature(engine.denoise_rings).parameters
    assert list(p) == ["frames", "fwd", "bwd", "sigma", "reach", "centre_weight", "return_stats"]
    assert [p[k].default for k in list(p)[4:]] == [1, 256, False]
    p = inspect.signature(engine.video_denoise_dense).parameters
    assert list(p)[-1] == "reach" and p["reach"].default == 1 and p["reach"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    # what existed kept its signature
    assert list(p)[:-1] == ["frames", "levels", "window", "sigma", "iters", "min_det", "max_px", "median", "mode", "centre_weight", "return_stats",
                            "return_displacements"]
    assert list(inspect.signature(engine._denoise_rings).parameters) == ["frames", "fwd", "bwd", "weights", "centre_weight", "return_stats"]
    assert "reach" not in inspect.signature(engine.video_denoise).parameters


@pytest.mark.parametrize("cc,flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_the_header_compiles_and_the_struct_has_the_bound_layout(tmp_path, cc, flags):
    from cuda_optical_flow_2_amd import lib

    desc_f = [f[0] for f in lib.ChainDesc._fields_]
    assert desc_f == ["d_link", "n_links", "w", "h", "mask_pitch", "d_dst", "d_mask", "d_stats"]
    check = "_Static_assert" if cc == "gcc" else "static_assert"
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include <assert.h>\n#include "ofx.h"\n'
           f'{check}(sizeof(ofx_chain_desc) == 72, "desc");\n{check}(offsetof(ofx_chain_desc, d_dst) == 48, "d_dst");\n'
           'int main(void){ofx_chain_desc c; (void)c;\n'
           'printf("%zu %zu %zu %zu %zu %d", sizeof(ofx_chain_desc), sizeof(c.d_link), sizeof(ofx_params), sizeof(ofx_temporal_desc),\n'
           '       sizeof(ofx_mosaic_desc), OFX_CHAIN_MAX_LINKS);\n'
           + "".join(f'printf(" %zu", offsetof(ofx_chain_desc, {f}));\n' for f in desc_f) + 'printf("\\n"); return 0;}\n')
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = tmp_path / "t"
    subprocess.run([cc, "-Wall", "-Werror"] + flags + [str(c), "-I", os.path.join(ROOT, "include"), "-o", str(exe)], check=True)
    s_desc, s_links, params, s_temporal, s_mosaic, max_n, *offs = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                                                                                   check=True).stdout.split())
    assert s_desc == C.sizeof(lib.ChainDesc) == 72 and s_links == 4 * 8 and max_n == 4
    assert offs == [getattr(lib.ChainDesc, f).offset for f in desc_f]
    assert params == C.sizeof(lib.Params) == 352, "sizeof(ofx_params) moved"
    assert s_temporal == C.sizeof(lib.TemporalDesc) == 144 and s_mosaic == C.sizeof(lib.MosaicDesc), "an earlier descriptor moved"


def test_abi_version_did_not_move():
    from cuda_optical_flow_2_amd import lib

    assert lib.load().ofx_abi_version() == 10


# made-up addresses: never dereferenced, every case below ends at a check on the host
LNK, DST, MASK, STATS = 0x40000000, 0x20000000, 0x28000000, 0x30000000
W_, H_, MP = 64, 48, 64 + 5
FIELD_BYTES = W_ * H_ * 8
MASK_BYTES = (H_ - 1) * MP + W_


def call(n=2, bad=1, L=3, link=None, items="ok", link_kw=None, first=None, **kw):
    """one ofx_displacement_chain call on n good items of L links; item `bad` gets kw, its link `link` the address link_kw (None: null); item 0
    gets `first` when it is not the bad one"""
    from cuda_optical_flow_2_amd import lib

    lib_ = lib.load()
    descs = (lib.ChainDesc * max(n, 1))()
    for i in range(max(n, 1)):
        d = descs[i]
        mine = i == min(bad, max(n, 1) - 1)
        C.memset(C.addressof(d), 0xEE, C.sizeof(d))       # garbage in the links >= L (and everywhere not set below)
        f = dict(n_links=L if mine or 2 <= L <= 4 else 3, w=W_, h=H_, mask_pitch=MP, d_dst=DST + (i << 20) + 8, d_mask=MASK + (i << 20) + 1,
                 d_stats=STATS + 128 * i)
        if mine:
            f.update(kw)
        elif i == 0 and first:
            f.update(first)
        for k, v in f.items():
            setattr(d, k, v)
        for k in range(max(0, min(d.n_links, 4))):
            d.d_link[k] = link_kw if mine and k == link else LNK + (i << 22) + (k << 17) + 8
    rc = lib_.ofx_displacement_chain(descs if items == "ok" else None, n, None)
    return rc, lib_.ofx_last_error()


def refused(word, item=1, link=None, **kw):
    rc, msg = call(link=link, **kw)
    assert rc == OFX_E_INVALID, (kw, rc)
    assert msg and word in msg and NAME.encode() in msg, (kw, msg)
    if item is not None:
        assert b"item %d" % item in msg, (kw, msg)
    else:
        assert b"item " not in msg, (kw, msg)
    if link is not None:
        assert b"link %d" % link in msg, (kw, msg)
    else:
        assert b"link " not in msg, (kw, msg)


def both_items(word, **kw):
    refused(word, item=1, **kw)
    refused(word, item=0, bad=0, **kw)


def both_links(word, L=3, links=None, **kw):
    """a refusal about a link: for link 0 (or `links`) and for the last one, for item 0 and for item 1"""
    for link in links or (0, L - 1):
        for bad in (0, 1):
            refused(word, item=bad, bad=bad, L=L, link=link, **kw)


def test_the_call_and_the_item_are_refused_before_anything_is_enqueued():
    refused(b"items is null", item=None, items=None)
    for n in (0, -1, 17, 1 << 20):
        refused(b"n =", item=None, n=n)
    for L in (1, 0, -1, 5, 1 << 20):
        both_items(b"n_links", L=L)
    both_items(b"d_dst is null", d_dst=None)
    for kw in (dict(w=0), dict(h=0), dict(w=-3), dict(h=-1)):
        both_items(b"size", **kw)
    both_items(b"w * h", w=1 << 14, h=1 << 14, mask_pitch=1 << 14)
    both_items(b"w * h", w=1 << 28, h=1, mask_pitch=1 << 28)
    for off in (4, 1, 12):
        both_items(b"d_dst must be 8-byte aligned", d_dst=DST + off)
        both_items(b"d_stats must be 8-byte aligned", d_stats=STATS + off)
    for mp in (W_ - 1, 0, -W_):
        both_items(b"mask_pitch", mask_pitch=mp)
    # the outputs against each other: the first and the last byte of either inside the other
    for bad in (0, 1):
        dst, mask = DST + (bad << 20) + 8, MASK + (bad << 20) + 1
        for at in (dst, dst + FIELD_BYTES - 1, dst - MASK_BYTES + 1):
            refused(b"d_mask and d_dst overlap", item=bad, bad=bad, d_mask=at)
        for at in (dst, dst + FIELD_BYTES - 8, dst - 24):
            refused(b"d_stats and d_dst overlap", item=bad, bad=bad, d_stats=at)
        for at in ((mask + 7) & ~7, (mask + MASK_BYTES - 1) & ~7, (mask - 31 + 7) & ~7):
            refused(b"d_stats and d_mask overlap", item=bad, bad=bad, d_stats=at)


def test_a_link_is_refused_with_its_number():
    for L in (2, 3, 4):
        both_links(b"d_link is null", L=L, link_kw=None)
        for off in (4, 1, 12):
            both_links(b"d_link must be 8-byte aligned", L=L, link_kw=LNK + off)
    for bad in (0, 1):
        dst, mask = DST + (bad << 20) + 8, MASK + (bad << 20) + 1
        for link in (0, 1, 3):
            # in place is link 0 at exactly d_dst: everything else that shares a byte with d_dst is refused
            for at in (dst + 8, dst - 8, dst + FIELD_BYTES - 8, dst - FIELD_BYTES + 8) + ((dst,) if link else ()):
                refused(b"d_link and d_dst overlap", item=bad, bad=bad, L=4, link=link, link_kw=at)
            for at in ((mask + MASK_BYTES - 1) & ~7, (mask - FIELD_BYTES + 8) & ~7):
                refused(b"d_link and d_mask overlap", item=bad, bad=bad, L=4, link=link, link_kw=at)


def test_what_is_allowed_passes_up_to_a_refused_last_check():
    """the last link's overlap with the mask is checked after everything else about an item: a call that reaches it has passed
    every other check -- in place on link 0 among them, which can be seen here without a launch"""
    dst = DST + (1 << 20) + 8
    allowed = [dict(L=4), dict(L=2), dict(w=1, h=1), dict(n=16, bad=15), dict(n=1, bad=0), dict(d_stats=None),
               dict(w=(1 << 14) - 1, h=1 << 14, mask_pitch=1 << 14, d_dst=0x100000000, d_stats=0x190000000),
               dict(link=0, link_kw=dst),                                                       # in place
               dict(link=0, link_kw=dst - FIELD_BYTES), dict(link=1, link_kw=dst + FIELD_BYTES),     # links that touch the destination
               dict(d_stats=dst + FIELD_BYTES), dict(d_stats=dst - 32)]
    for kw in allowed:
        kw = dict(kw)
        L = kw.get("L", 3)
        w, h, mp = kw.get("w", W_), kw.get("h", H_), kw.get("mask_pitch", MP)
        mask = MASK + (kw.get("bad", 1) << 20) + 1
        first_link, first_kw = kw.pop("link", None), kw.pop("link_kw", None)
        if first_link is not None:                           # the address under test goes in through the descriptor's own link
            ok = call_with(kw, L, first_link, first_kw, last=(mask + (h - 1) * mp + w - 1) & ~7)
        else:
            ok = call(link=L - 1, link_kw=(mask + (h - 1) * mp + w - 1) & ~7, **kw)
        rc, msg = ok
        assert rc == OFX_E_INVALID and NAME.encode() in msg and b"d_link and d_mask overlap" in msg, (kw, msg)
        assert b"item %d" % kw.get("bad", 1) in msg and b"link %d" % (L - 1) in msg, (kw, msg)
    # d_stats NULL in item 0: the call gets as far as item 1, which is refused
    rc, msg = call(first=dict(d_stats=None), d_stats=STATS + 4)
    assert rc == OFX_E_INVALID and b"d_stats" in msg and b"item 1" in msg, msg
    # without a mask its pitch is not looked at: the refusal is a later one
    rc, msg = call(d_mask=None, mask_pitch=0, link=2, link_kw=LNK + 4)
    assert rc == OFX_E_INVALID and b"link 2: d_link must be 8-byte aligned" in msg, msg


def call_with(kw, L, link, addr, last):
    """call() with two links of the bad item set: `link` to addr and the last one to `last`"""
    from cuda_optical_flow_2_amd import lib

    lib_ = lib.load()
    n, bad = kw.get("n", 2), kw.get("bad", 1)
    descs = (lib.ChainDesc * n)()
    for i in range(n):
        d = descs[i]
        C.memset(C.addressof(d), 0xEE, C.sizeof(d))
        d.n_links, d.w, d.h, d.mask_pitch, d.d_dst, d.d_mask, d.d_stats = L, W_, H_, MP, DST + (i << 20) + 8, MASK + (i << 20) + 1, STATS + 128 * i
        for k in range(L):
            d.d_link[k] = LNK + (i << 22) + (k << 17) + 8
        if i == bad:
            d.d_link[link], d.d_link[L - 1] = addr, last
    rc = lib_.ofx_displacement_chain(descs, n, None)
    return rc, lib_.ofx_last_error()
