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
        for k in ("stats", "outside", "info", "model", "status", "points", "count", "cells", "flow0"):      # what lies in a shared buffer
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
