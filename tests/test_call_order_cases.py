"""CPU: the recipes of tests/call_order_cases.py by the referees alone -- every recipe builds and its `want` computes, each reaches what
its row of the table claims (two score tiles, two hypothesis groups, refits that ran, usable and unusable matches, pixels inside and
outside, points tracked and lost, cells with and without a feature), and the results of the calls that share buffers on the device
differ from one another, so that an output left over from the first call cannot pass for the second's."""
import numpy as np
import pytest

import call_order_cases as CC
import fit_motion_ref as FR
import homography_ref as HR


@pytest.mark.parametrize("name", CC.NAMES)
def test_every_recipe_builds_and_its_referee_answers(name):
    r = CC.recipe(name)
    assert r.name == name and r.entry.startswith("ofx_") and r.want
    for k, w in r.want.items():
        assert isinstance(w, np.ndarray) and w.size > 0, (name, k)
        assert w.dtype in (np.uint8, np.int32, np.int64, np.float32, np.float64), (name, k, w.dtype)
    for attr in ("stage", "launch", "outputs", "read"):
        assert callable(getattr(r, attr))


def test_wipe_overwrites_structures_tables_and_arrays():
    import ctypes as C

    prm = CC.L.FitParams(1, 2, 3, 4, 5)
    table = (C.c_void_p * 3)(1, 2, 3)
    arr = np.arange(4, dtype=np.float32)
    CC.wipe(prm, table, arr, None)
    assert prm.model == -1 and prm.seed == 0xFFFFFFFF and list(table) == [2 ** 64 - 1] * 3 and (arr.view(np.uint8) == 0xFF).all()


@pytest.mark.parametrize("model", CC.MODELS + ("homography",))
def test_the_fits_split_the_work_and_meet_both_kinds_of_match(model):
    for r in (CC.recipe(f"fit-{model}"),) + ((CC.other(f"fit-{model}"),) if f"fit-{model}" in CC.OTHERS else ()):
        assert r.reach["tiles"] >= 2 and r.reach["groups"] >= 2
        assert r.reach["n"] == [1025, 65] and r.reach["status"] == [False, True]
        for info, n in zip(r.reach["info"], r.reach["n"]):
            assert info[0] == FR.FIT_OK and 0 < info[1] < n and info[6] == r.prm[2] and 0 < info[5] < info[1]
    r = CC.recipe(f"fit-{model}")
    assert r.prm[0] == 33 and r.prm[2] == 2 and all(info[6] == 2 for info in r.reach["info"])
    # the status array of the second item matters: without it more matches are usable
    p, q, st, pair, size = r.items[1]
    assert int(FR.lattice(p, q, size, None, pair)[2].sum()) > r.reach["info"][1][1]
    assert all(0 < r.want[f"mask{i}"].sum() < r.want[f"mask{i}"].size for i in (0, 1))


@pytest.mark.parametrize("name", ["warp-affine", "warp-perspective"])
def test_the_warps_leave_pixels_outside_and_inside(name):
    for r in (CC.recipe(name), CC.other(name)):
        assert r.reach["channels"] == [3, 1] and [it[1] for it in r.items] == [(67, 45)] * 2 and [it[0].shape[:2] for it in r.items] == [(48, 64)] * 2
        assert all(it[3] == "constant" for it in r.items)
        assert all(0 < n < px for n, px in zip(r.reach["outside"], r.reach["pixels"]))
        assert 67 * 45 > 256 * 4, "more than one block of 256 quads"


def test_the_tracker_tracks_some_points_and_loses_others():
    for r in (CC.recipe("tracker"), CC.other("tracker")):
        assert r.reach["tracked"] > 0 and r.reach["lost"] > 0 and r.reach["n"] == 40 and len(r.frames) == 3
        assert set(np.unique(r.want["status"][r.start[1] == 0] & 255)) >= {0, 1}
        assert (r.want["sad"] >= 0).any() and (r.want["sad"] == -1).any() and r.want["stats"].shape == (2, 7)
        assert r.want["stats"][1, 0] > 0, "points are alive after the last pair"


def test_the_features_have_cells_with_and_without_one():
    r = CC.recipe("features")
    assert 0 < r.reach["occupied"] < r.reach["cells"] == 7 * 4
    assert int(r.want["count"][0]) == r.reach["occupied"] and (r.want["cells"][..., 0] == -1).any()
    assert (r.want["points"][r.reach["occupied"]:].view(np.uint8) == CC.FILL).all(), "entries beyond the count are left alone"


def test_the_other_recipes_meet_their_special_cases():
    assert all(t[0] * t[1] >= 2 for t in CC.recipe("median").reach["tiles"])
    for name in ("interp", "interp-colour", "consistency"):
        assert all(c > 0 for c in CC.recipe(name).reach["classes"]), name
        assert len(CC.recipe(name).pairs) == 2
    assert len(CC.recipe("interp").times) == 3
    assert 0 < CC.recipe("motion").reach["not_warped"] < 67 * 45
    assert CC.recipe("sampled").reach["moved"] > 0 and CC.recipe("sampled").reach["lost"] > 0
    assert (CC.recipe("sampled").want["arrows"][..., 2] == -1).any(), "an arrow that is not drawn"
    assert not np.isfinite(CC.recipe("displacement").want["disp"]).all()
    for mode in ("lk_float", "compat_cpu"):
        assert CC.recipe(f"lk-pair-{mode}").reach["nonfinite"] > 0
    assert CC.differs(CC.recipe("lk-pair-lk_float").want, CC.recipe("lk-pair-compat_cpu").want)
    f = CC.recipe("frontend")
    assert f.modes == [CC.GREY, CC.BILATERAL] and f.win == 5


@pytest.mark.parametrize("name", list(CC.OTHERS))
def test_two_calls_in_flight_have_different_answers(name):
    a, b = CC.recipe(name), CC.other(name)
    assert a.entry == b.entry and CC.differs(a.want, b.want)
    shared = [k for k in a.want if k in b.want and a.want[k].shape == b.want[k].shape]
    assert shared and all(a.want[k].tobytes() != b.want[k].tobytes() for k in shared if not k.startswith("plane")), name


@pytest.mark.parametrize("name", list(CC.CHAINS))
def test_calls_that_share_buffers_have_different_answers(name):
    chain = CC.chain(name)
    assert len(chain) >= 2 and len({r.entry for r in chain}) == 1
    for a, b in zip(chain, chain[1:]):
        for k in ("stats", "outside", "info", "model", "status", "points", "count", "cells", "flow0", "counts", "which0", "which1", "which4"):      # what lies in a shared buffer
            if k in a.want and k in b.want:
                assert a.want[k].tobytes() != b.want[k].tobytes(), f"{name}: {a.name} and {b.name} agree in {k}"
        assert CC.differs(a.want, b.want)


@pytest.mark.parametrize("model", CC.MODELS + ("homography",))
def test_the_fit_chain_is_the_issues(model):
    chain = CC.chain(f"fit-{model}")
    K = (HR.HOMOGRAPHY if model == "homography" else FR.MODELS[model]) + 1
    assert chain[0].prm[:3] == (256, 32, 3) and chain[0].reach["n"] == [4099] and chain[0].reach["info"][0][6] == 3
    assert chain[1].prm[0] == 33 and chain[1].prm[2] == 0 and chain[1].reach["n"] == [65] and chain[1].prm[3] != chain[0].prm[3]
    assert chain[1].reach["status"] == [True] and 0 < chain[1].reach["info"][0][1] < 65
    assert chain[2].reach["info"][0][1] == 3, "three usable matches"
    few = chain[-1]
    assert few.reach["info"][0][1] == min(3, K - 1) and few.reach["info"][0] == [FR.FIT_FEW, min(3, K - 1), 0, -1, 0, 0, 0, 0]
    ident = HR.IDENTITY if model == "homography" else FR.IDENTITY
    assert few.want["model"].reshape(-1).tolist() == list(ident) and not few.want["mask0"].any()
    assert (len(chain) == 3) == (model == "homography")


def test_the_warp_chain_goes_from_many_pixels_outside_to_none():
    for name in ("warp-affine", "warp-perspective"):
        a, b = CC.chain(name)
        assert all(n > 67 * 45 // 2 for n in a.reach["outside"]) and b.reach["outside"] == [0, 0]


def test_the_tracker_chain_is_the_whole_chain_cut_in_two():
    whole = CC.recipe("tracker")
    a, b = CC.chain("tracker")
    assert (a.pair0, b.pair0) == (1, 2)
    CC.same(b.want["points"], whole.want["points"], "points")
    CC.same(b.want["status"], whole.want["status"], "status")
    CC.same(np.concatenate([a.want["stats"], b.want["stats"]]), whole.want["stats"], "stats")


def test_the_second_feature_image_is_smaller_and_keeps_the_firsts_surroundings():
    a, b = CC.chain("features")
    assert b.w < a.w and b.h < a.h and b.ncx < a.ncx and b.ncy < a.ncy
    assert np.array_equal(b.want["strength"][b.h:], a.want["strength"][b.h:]) and np.array_equal(b.want["strength"][:, b.w:], a.want["strength"][:, b.w:])
    assert not np.array_equal(b.want["strength"][:b.h, :b.w], a.want["strength"][:b.h, :b.w])
    n = b.ncx * b.ncy
    assert np.array_equal(b.want["cells"].reshape(-1, 2)[n:], a.want["cells"].reshape(-1, 2)[n:])
    assert int(b.want["count"][0]) < int(a.want["count"][0])
    k = int(b.want["count"][0])
    assert np.array_equal(b.want["points"][k:int(a.want["count"][0])], a.want["points"][k:int(a.want["count"][0])]), "the first call's points stay"


# ---- the frame mosaic -------------------------------------------------------------------------------------------------------------------
def test_the_mosaic_takes_the_widest_instances_and_meets_every_bin():
    for r in (CC.recipe("mosaic"), CC.other("mosaic")):
        assert len(r.items) == 5 > 4, "more than four items: the 16-item instance"
        assert max(r.reach["sources"]) == 6 > 5 and min(r.reach["sources"]) == 1, "more than five sources: the 9-source instance"
        assert len({(it[2], r.reach["channels"][i]) for i, it in enumerate(r.items)}) == 5 and set(r.reach["channels"]) == {1, 3}
        assert {(w, g) for w, g in zip(r.reach["which"], r.reach["given"])} == {(True, True), (True, False), (False, True), (False, False)}
        assert all(sum(c) == px for c, px in zip(r.reach["counts"], r.reach["pixels"]))
        assert any(c[9] > 0 for c in r.reach["counts"]), "a pixel that nobody covers"
        assert any(sum(c[1:9]) > 0 for c in r.reach["counts"]) and any(c[5] > 0 for c in r.reach["counts"]), "a source that is not the first, and the sixth"
        assert 67 * 45 > 256 * 4, "more than one block of 256 quads"
        # the slots of the items that gave no d_counts keep their 0x5A
        for i, given in enumerate(r.reach["given"]):
            assert (r.want["counts"][i, 0].tolist() == r.reach["counts"][i]) == given
            assert given or (r.want["counts"][i].view(np.uint8) == CC.FILL).all()
        assert sorted(k for k in r.want if k.startswith("which")) == [f"which{i}" for i, w in enumerate(r.reach["which"]) if w]
    r = CC.recipe("mosaic")
    assert all(c[9] > 0 for c in r.reach["counts"]), "the ladder leaves its last band to nobody"
    for k in ("which0", "which1", "which4"):
        assert set(np.unique(r.want[k])) >= {0, 255}


def test_the_mosaic_chain_goes_from_few_pixels_covered_to_most():
    a, b = CC.chain("mosaic")
    assert [it[2:] for it in a.items] == [it[2:] for it in b.items], "the same sizes, borders, fills and outputs: the buffers are shared"
    for ca, cb, px, S in zip(a.reach["counts"], b.reach["counts"], a.reach["pixels"], a.reach["sources"]):
        assert 0 < px - ca[9] < px // 3 and px - cb[9] > px // 2, (ca, cb, px)     # less than a third, then more than half
        assert S == 1 or (ca[1] > 0 and cb[1] > 0), "a source that is not the first, in both calls"
        assert all(x != y for x, y in zip(ca, cb) if x or y), "every bin that either call fills differs: a bin that is not zeroed again shows"


class _Buffer:
    """what Mosaic.launch asks of a staged input or output"""

    def __init__(self, ptr, pitch):
        self.ptr, self.pitch = ptr, pitch

    def slot(self, i):
        return self.ptr + 80 * i


class _Library:
    def ofx_warp_mosaic(self, descs, n, stream):
        self.descs, self.n, self.stream, self.seen = descs, n, stream, bytes(descs)
        return 0


def _mosaic_call(r):
    """r.launch against a library that records: (the descriptors as the library saw them, their bytes after the call)"""
    lib = _Library()
    r.lib = lambda: lib
    r.table, r.outs, at = [], {}, 0x1000
    for i, (srcs, models, (w, h), border, fill, which, cnt) in enumerate(r.items):
        ch = r.reach["channels"][i]
        r.table.append([_Buffer(at + 0x100 * k + 1, ch * s.shape[1] + 5 + k) for k, s in enumerate(srcs)])
        r.outs[f"dst{i}"] = _Buffer(at + 0x1000 + 3, ch * w + 7)
        r.outs[f"which{i}"] = _Buffer(at + 0x2000 + 1, w + 3)
        at += 0x10000
    r.outs["counts"] = _Buffer(0x900008, 10)
    try:
        assert r.launch(0x77) == 0 and lib.n == len(r.items) and lib.stream == 0x77
    finally:
        del r.lib, r.table
        r.outs = {}
    return (CC.L.MosaicDesc * lib.n).from_buffer_copy(lib.seen), bytes(lib.descs)


def test_the_mosaic_launch_builds_its_descriptors_and_wipes_them():
    r = CC.recipe("mosaic")
    seen, after = _mosaic_call(r)
    assert set(after) == {0xFF}, "the host array is overwritten as soon as the call has returned"
    for i, (d, (srcs, models, (w, h), border, fill, which, cnt)) in enumerate(zip(seen, r.items)):
        assert (d.n_sources, d.w, d.h, d.channels, d.fill) == (len(srcs), w, h, r.reach["channels"][i], fill)
        assert (d.d_which is not None) == which and (d.d_counts is not None) == cnt and (which or d.which_pitch == -1)
        assert d.d_counts in (None, 0x900008 + 80 * i) and (d.d_counts or 0) % 8 == 0
        for k, (s, m) in enumerate(zip(srcs, models)):
            assert (d.source[k].sw, d.source[k].sh) == (s.shape[1], s.shape[0]) and list(d.source[k].model) == [float(x) for x in m]
            assert d.source[k].d_src % 2 == 1, "an odd address"
    # the variant hands the library the very same bytes
    assert bytes(_mosaic_call(CC.variant("mosaic"))[0]) == bytes(seen)


# ---- the variants -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.NAMES)
def test_a_variant_has_another_answer_and_reaches_the_same_branches(name):
    r, v = CC.recipe(name), CC.variant(name)
    assert v is not r and type(v) is type(r) and v.entry == r.entry
    assert set(v.want) == set(r.want) and all(v.want[k].shape == r.want[k].shape and v.want[k].dtype == r.want[k].dtype for k in r.want), "the same geometry"
    assert CC.differs(r.want, v.want), f"{name}: the variant's answer is the recipe's: a replay that read nothing anew would pass"
    assert r.branches() == v.branches(), (name, r.branches(), v.branches())       # (what the recipe reaches: the tests above)
    # the call made on outputs that hold the variant's results: only the feature points beyond the count keep anything of them
    over = r.want_over(v)
    assert set(over) == set(r.want) and all(over[k] is r.want[k] for k in r.want if (name, k) != ("features", "points"))
    if name == "features":
        n, m = r.reach["occupied"], v.reach["occupied"]
        assert n < m, "the variant finds more points: some of them stay behind the recipe's"
        assert np.array_equal(over["points"][:n], r.want["points"][:n]) and np.array_equal(over["points"][n:], v.want["points"][n:])
        assert not np.array_equal(over["points"], r.want["points"])


def test_the_variants_pass_the_same_host_arguments():
    """what the constructors keep of the host's side, row by row"""
    for name in CC.NAMES:
        r, v = CC.recipe(name), CC.variant(name)
        for attr in ("model", "prm", "pair0", "levels", "w", "h", "border", "max_points", "coarse", "fine", "colour", "pair", "mode", "L", "win", "modes"):
            assert getattr(r, attr, None) == getattr(v, attr, None), (name, attr)
        for attr in ("times",):
            assert np.array_equal(getattr(r, attr, 0), getattr(v, attr, 0)), (name, attr)
    for name in ("fit-affine", "fit-homography"):
        for a, b in zip(CC.recipe(name).items, CC.variant(name).items):
            assert (len(a[0]), a[2] is None, a[3], a[4]) == (len(b[0]), b[2] is None, b[3], b[4]), "n, status given, pair, frame size"
    for name in ("warp-affine", "warp-perspective"):
        assert [it[1:] for it in CC.recipe(name).items] == [it[1:] for it in CC.variant(name).items], "sizes, models, borders, fills"
    assert [it[1:] for it in CC.recipe("median").items] == [it[1:] for it in CC.variant("median").items], "w, h, radius"
    assert [len(f) for f in (CC.recipe("tracker").frames, CC.variant("tracker").frames)] == [3, 3]
    assert [len(r.start[0]) for r in (CC.recipe("tracker"), CC.variant("tracker"), CC.recipe("sampled"), CC.variant("sampled"))] == [40] * 4
    assert [it[1:] for it in CC.recipe("mosaic").items] == [it[1:] for it in CC.variant("mosaic").items], "models, sizes, borders, fills, outputs"
