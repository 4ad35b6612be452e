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
    # (the chain of a 1 x 1 field leaves the frame unless link 0 is exactly zero: both answers are the dead vector)
    assert shared and all(a.want[k].tobytes() != b.want[k].tobytes() for k in shared if not k.startswith("plane") and (name, k) != ("chain", "dst4")), name


@pytest.mark.parametrize("name", list(CC.CHAINS))
def test_calls_that_share_buffers_have_different_answers(name):
    chain = CC.chain(name)
    assert len(chain) >= 2 and len({r.entry for r in chain}) == 1
    for a, b in zip(chain, chain[1:]):
        for k in ("stats", "outside", "info", "model", "status", "points", "count", "cells", "flow0", "counts", "which0", "which1", "which4", "dst0", "mask0",
                  "fwd2", "bwd2", "frames"):      # what lies in a shared buffer
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
        for attr in ("model", "prm", "pair0", "levels", "w", "h", "border", "max_points", "coarse", "fine", "colour", "pair", "mode", "L", "win", "modes",
                     "slots", "carried", "wc", "channels"):
            assert getattr(r, attr, None) == getattr(v, attr, None), (name, attr)
        for attr in ("times", "weights"):
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


# ---- the displacement chain, the temporal filter, and the two together ------------------------------------------------------------------
class _Arena:
    """addresses that depend on the order and the sizes of the requests alone, 512 bytes aligned as a device allocation is"""

    def __init__(self):
        self.at = 0x100000

    def take(self, nbytes):
        at = self.at
        self.at += (nbytes + 511) // 512 * 512 + 512
        return at


def _fakes(arena):
    """stand-ins for call_order_cases.In, InOut and Guarded that hold addresses and no memory"""
    class In:
        def __init__(self, torch, host, lead=0, tail=16):
            host = np.asarray(host)
            self.ptr = arena.take((lead + host.size + tail) * host.itemsize) + lead * host.itemsize

        @classmethod
        def plane(cls, torch, arr, pitch, lead, around):
            self = cls.__new__(cls)
            assert arr.ndim == 2 and pitch >= arr.shape[1]
            self.ptr, self.pitch, self.rows = arena.take(lead + arr.shape[0] * pitch + 64) + lead, pitch, arr.shape[0]
            return self

    class InOut:
        def __init__(self, torch, g, host):
            assert g.n == 1 and g.pitch == g.w and np.asarray(host).size == g.rows * g.w

    class Guarded:
        def __init__(self, dtype, n, rows, w, pitch, lead, stride=None):
            self.n, self.rows, self.w, self.pitch, self.lead = n, rows, w, pitch, lead
            self.stride = rows * pitch + 20 if stride is None else stride
            self.size = np.dtype(dtype).itemsize
            self.ptr = arena.take((lead + n * self.stride + 64) * self.size) + lead * self.size

        def slot(self, i):
            return self.ptr + i * self.stride * self.size

    return In, InOut, Guarded


class _Recorder:
    """the two entry points, recording what they were handed as it was during the call"""

    def __init__(self):
        self.calls = []

    def ofx_displacement_chain(self, descs, n, stream):
        self.calls.append(dict(entry="chain", descs=descs, seen=bytes(descs), n=n, stream=stream, prm=None, prm_seen=b""))
        return 0

    def ofx_temporal_filter(self, descs, n, prm, stream):
        self.calls.append(dict(entry="temporal", descs=descs, seen=bytes(descs), n=n, stream=stream, prm=prm._obj, prm_seen=bytes(prm._obj)))
        return 0


def _recorded(monkeypatch, r, share=None):
    """r staged on addresses alone (its own stage()), launched against the recorder: the calls, each with the descriptors
    (`descs`: as the library saw them) and the bytes of the host arrays once the call was back (`after`); and the staged recipe's
    outputs, which are addresses"""
    In, InOut, Guarded = _fakes(_Arena())
    lib = _Recorder()
    before = dict(vars(r))          # the recipe is cached: whatever stage() sets on it is taken off again
    with monkeypatch.context() as m:
        for k, v in (("In", In), ("InOut", InOut), ("Guarded", Guarded)):
            m.setattr(CC, k, v)
        r.lib = lambda: lib
        try:
            r.stage(None)
            assert r.launch(0x77) == 0
            outs, ins = dict(r.outs), list(r.ins)
        finally:
            vars(r).clear()
            vars(r).update(before)
    for c in lib.calls:
        assert c["stream"] == 0x77
        c["after"] = bytes(c["descs"]) + (bytes(c["prm"]) if c["prm"] is not None else b"")
        Desc = CC.L.ChainDesc if c["entry"] == "chain" else CC.L.TemporalDesc
        c["descs"] = (Desc * c["n"]).from_buffer_copy(c["seen"])
        if c["prm"] is not None:
            c["prm"] = CC.L.TemporalParams.from_buffer_copy(c["prm_seen"])
    return lib.calls, outs, ins


@pytest.mark.parametrize("name", ["chain", "temporal", "temporal-one", "denoise-reach2"])
def test_the_new_rows_pass_the_same_bytes_and_wipe_them(monkeypatch, name):
    """recipe and variant staged on buffers whose addresses depend on the geometry alone: the library sees identical descriptors and
    parameters, they read 0xFF once the call is back, and the fixed-size slots beyond n_links and n_neighbours are zero"""
    calls, _, _ = _recorded(monkeypatch, CC.recipe(name))
    again, _, _ = _recorded(monkeypatch, CC.variant(name))
    assert [c["entry"] for c in calls] == [c["entry"] for c in again] == {"chain": ["chain"], "denoise-reach2": ["chain", "temporal"]}.get(name, ["temporal"])
    for c, v in zip(calls, again):
        assert c["seen"] == v["seen"] and c["prm_seen"] == v["prm_seen"] and c["n"] == v["n"], f"{name}: the variant passes other host arguments"
        assert c["after"] and set(c["after"]) == {0xFF}, f"{name}: a host array is not overwritten once the call is back"
        for d in c["descs"]:
            if c["entry"] == "chain":
                assert 2 <= d.n_links <= 4 and all(d.d_link[k] for k in range(d.n_links)) and not any(d.d_link[k] for k in range(d.n_links, 4))
                # (a ring's slots are 17688 bytes apart: they alternate)
                assert all(a % 16 == 8 or (name != "chain" and a % 8 == 0) for a in [d.d_link[k] for k in range(d.n_links)] + [d.d_dst]), "fields sit 8 but not 16 bytes in"
            else:
                assert 1 <= d.n_neighbours <= 4
                for k, s in enumerate(d.neighbour):
                    assert (k < d.n_neighbours) == bool(s.d_plane) == bool(s.d_field) and (k < d.n_neighbours or (s.pitch, s.pad) == (0, 0))
                    assert not s.d_field or s.d_field % 16 == 8 or (name == "denoise-reach2" and s.d_field % 8 == 0)
        if c["prm"] is not None:
            r = CC.recipe(name)
            assert list(c["prm"].weights) == r.weights.tolist() and (c["prm"].centre_weight, c["prm"].reserved) == (r.wc, 0)


def test_the_chain_launch_builds_the_issues_descriptors(monkeypatch):
    r = CC.recipe("chain")
    (call,), outs, _ = _recorded(monkeypatch, r)
    assert call["n"] == 6
    for i, (d, (w, h, n, mask, given, there)) in enumerate(zip(call["descs"], CC.CHAIN_GEOM)):
        assert (d.w, d.h, d.n_links) == (w, h, n) and d.d_dst == outs[f"dst{i}"].ptr
        assert (d.d_link[0] == d.d_dst) == there and len({d.d_link[k] for k in range(n)} | {d.d_dst}) == n + (not there)
        assert (d.d_stats is not None) == given and (d.d_stats or 0) % 8 == 0 and d.d_stats in (None, outs["stats"].ptr + 32 * i), "item i at slot i, 32 bytes apart"
        if mask is None:
            assert d.d_mask is None and d.mask_pitch == -1
        elif mask == "loose":
            assert d.d_mask % 4 == 0 and d.mask_pitch % 4 == 0 and d.mask_pitch > w
        else:
            assert d.d_mask % 2 == 1 and d.mask_pitch % 2 == 1 and d.mask_pitch > w


def _zeroing_runs(slots, words):
    """a restatement, for the layout of the staged addresses only (the library is held by the guard and slot bytes on the GPU), of
    the launches of quad_stage.h's zero_stats on the addresses `slots` (None: not given), `words` 64-bit words each: a run is a
    slot and the given slots that follow it at ascending consecutive addresses"""
    runs, i = [], 0
    while i < len(slots):
        e = i + 1
        if slots[i] is not None:
            while e < len(slots) and slots[e] == slots[i] + 8 * words * (e - i):
                e += 1
            runs.append((i, e))
        i = e
    return runs


def _slot_addresses(monkeypatch, r):
    (call,), _, _ = _recorded(monkeypatch, r)
    return [d.d_stats for d in call["descs"]]


def test_the_stats_slots_make_three_runs_four_single_launches_and_one(monkeypatch):
    """what zero_stats (csrc/quad_stage.h) makes of the slots: 0 | 2, 3 | 5 in the row -- a merged run between two gaps --, every slot
    on its own where the addresses descend, and the fold's one slot"""
    assert _zeroing_runs(_slot_addresses(monkeypatch, CC.recipe("chain")), 4) == [(0, 1), (2, 4), (5, 6)]
    assert _zeroing_runs(_slot_addresses(monkeypatch, CC.variant("chain")), 4) == [(0, 1), (2, 4), (5, 6)]
    other = _slot_addresses(monkeypatch, CC.other("chain"))
    given = [a for a in other if a is not None]
    assert given == sorted(given, reverse=True) and given[1] - given[2] == 32, "descending, two of them neighbours in memory"
    assert _zeroing_runs(other, 4) == [(0, 1), (2, 3), (3, 4), (5, 6)]
    for r in CC.chain("chain"):
        assert _zeroing_runs(_slot_addresses(monkeypatch, r), 4) == [(0, 1)]
    assert _zeroing_runs([None, 64, 96, None, 160, 128, None], 4) == [(1, 3), (4, 5), (5, 6)]


@pytest.mark.parametrize("make", [CC.recipe, CC.variant, CC.other], ids=["recipe", "variant", "other"])
def test_the_chain_row_reaches_what_the_issue_names(make):
    r = make("chain")
    R = r.reach
    assert R["sizes"] == [(257, 40), (67, 33), (130, 9), (5, 3), (1, 1), (67, 33)] and R["links"] == [3, 2, 4, 2, 2, 4] and set(R["links"]) == {2, 3, 4}
    assert R["masks"] == ["odd", "loose", None, "odd", None, "loose"] and R["given"] == [True, False, True, True, False, True] and sum(R["there"]) == 2
    assert -(-257 // 4) * 40 > 2 * 256 * 4, "257 x 40: more than two blocks of 256 threads and four quads each"
    assert all(s[0] == w * h == sum(s[1:]) for s, (w, h) in zip(R["stats"], R["sizes"]))
    for i, given in enumerate(R["given"]):
        slot = r.want["stats"][r.slots[i], 0]
        assert (slot.tolist() == R["stats"][i]) == given and (given or (slot.view(np.uint8) == CC.FILL).all()), "a slot that was not given keeps its 0x5A"
    assert (r.slots == list(range(6))) == (make is not CC.other) and sorted(r.slots) == list(range(6))
    # the 1 x 1 item leaves the frame in all three: its dst is the dead vector and cannot tell them apart (that is why
    # test_two_calls_in_flight_have_different_answers leaves dst4 out); should it ever become defined, take the exemption away
    assert R["stats"][4] == [1, 1, 0, 0] and r.want["dst4"].view(np.uint32).tolist() == [[[CC.KR.DEAD_BITS] * 2]]
    if make is CC.other:
        return
    assert all(c > 0 for c in R["stats"][5][1:]), "67 x 33 overflow: leaves, undefined and ok"
    assert make is not CC.recipe or R["stats"][5] == [2211, 309, 1881, 21]
    assert R["stats"][0][1] > 0 and R["stats"][0][3] > 0 and R["stats"][2][2] > 0, "257 x 40: leaves and ok; 130 x 9 edge: undefined"


def test_the_chain_fold_ends_at_the_chain_of_all_four_links():
    fold = CC.chain("chain")
    links = CC.KC.links("borders", 257, 40, 4)
    dst, cls, stats = CC.KR.chain(list(links))
    CC.same(fold[-1].want["dst0"].reshape(40, 257, 2), dst, "the last call of the fold")
    assert [r.carried for r in fold] == [False, True, True] and all(r.items[0][1:] == ("odd", True, True) for r in fold)
    assert [r.reach["stats"][0] for r in fold] == [[10280, 3681, 0, 6599], [10280, 3722, 3681, 2877], [10280, 1633, 7403, 1244]]
    for a, b in zip(fold, fold[1:]):
        assert all(x != y for x, y in zip(a.reach["stats"][0][1:], b.reach["stats"][0][1:])), "every bin but the pixel count differs between consecutive calls"
        assert b.items[0][0][0].tobytes() == a.want["dst0"].tobytes(), "link 0 of a call is the answer of the call before"


@pytest.mark.parametrize("make", [CC.recipe, CC.variant, CC.other], ids=["recipe", "variant", "other"])
def test_the_temporal_row_reaches_what_the_issue_names(make):
    r = make("temporal")
    R = r.reach
    assert R["sizes"] == [(131, 9), (67, 9), (5, 3), (67, 9), (3, 2), (131, 9)] and R["channels"] == [1, 3, 1, 1, 3, 3] and R["neighbours"] == [4, 2, 1, 3, 2, 3]
    assert R["given"] == [True, True, False, True, False, True] and R["same"] == [False, False, False, True, False, False] and R["own"] == [False] * 4 + [True, False]
    assert len(r.items) == 6 > 1, "more than one item: the 16-item instance"
    assert -(-131 // 4) * 9 > 256, "131 x 9: more than one block of 256 quads"
    for i in (0, 3, 5):
        px, s = R["sizes"][i][0] * R["sizes"][i][1], R["stats"][i]
        assert all(0 < u < px for u in s[1:1 + R["neighbours"][i]]) and all(u == 0 for u in s[1 + R["neighbours"][i]:5]), (i, s)
    assert all(u > 0 for u in R["stats"][0][1:5])
    for i, (given, it) in enumerate(zip(R["given"], r.items)):
        assert not given or (R["stats"][i][5] > 0 and R["stats"][i][6] > 0), (i, R["stats"][i])
        assert r.want[f"dst{i}"].tobytes() != np.ascontiguousarray(it[1]).tobytes(), f"item {i}: the output is the centre"
        slot = r.want["stats"][i, 0]
        assert (slot.tolist() == R["stats"][i]) == given and (given or (slot.view(np.uint8) == CC.FILL).all())
    if make is CC.other:
        assert (r.wc, r.weights.tolist()) == (256, CC.TC.tables()["sigma 10"].tolist())
    else:
        assert (r.wc, r.weights.tolist()) == (37, CC.TC.tables()["random"].tolist())


def test_the_temporal_rows_planes_start_at_every_address_mod_4(monkeypatch):
    _, _, ins = _recorded(monkeypatch, CC.recipe("temporal"))
    planes = [p for p in ins if hasattr(p, "pitch")]
    assert len(planes) == 6 + (4 + 2 + 1 + 3 + 2 + 3) - 2, "a plane per centre and neighbour, the `same` and the `own` one staged once"
    assert all(p.pitch % 2 == 1 for p in planes)
    assert all({(p.ptr + y * p.pitch) % 4 for y in range(p.rows)} == {0, 1, 2, 3} for p in planes if p.rows >= 4)
    assert {p.ptr % 4 for p in planes} == {0, 1, 2, 3}


def test_temporal_one_is_the_first_item_alone():
    for make in (CC.recipe, CC.variant):
        one, six = make("temporal-one"), make("temporal")
        assert len(one.items) == 1 and one.branches()["instance"] == 1 and six.branches()["instance"] == 16 and one.reach["given"] == [True]
        CC.same(one.want["dst0"], six.want["dst0"], "dst0")
        CC.same(one.want["stats"][0], six.want["stats"][0], "stats")


def test_the_temporal_chain_goes_through_no_weight_at_all():
    a, b, c = CC.chain("temporal")
    T = CC.TC.tables()
    assert [(r.weights.tolist(), r.wc) for r in (a, b, c)] == [(T["all 256"].tolist(), 1), (T["all 0"].tolist(), 256), (T["sigma 10"].tolist(), 256)]
    for r in (a, b, c):
        assert r.reach["sizes"] == [(131, 9), (67, 9), (131, 9)] and r.reach["channels"] == [1, 1, 3] and r.reach["given"] == [True] * 3
        assert not any("ramp" in it[0] for it in r.items)
    for i, (s, (w, h)) in enumerate(zip(b.reach["stats"], b.reach["sizes"])):
        assert s[5] == w * h and s[6] == s[7] == 0, "no weight anywhere: every pixel is left as it was"
        assert b.want[f"dst{i}"].tobytes() == np.ascontiguousarray(b.items[i][1]).tobytes()
    for x, y in ((a, b), (b, c)):
        for sx, sy in zip(x.reach["stats"], y.reach["stats"]):
            assert all(p != q for p, q in zip(sx[1:], sy[1:]) if p or q), f"{x.name}, {y.name}: a bin that is not zeroed again would not show: {sx} {sy}"


def test_the_denoise_row_chains_through_undefined_vectors_and_fills_every_neighbour_bin():
    for r in (CC.recipe("denoise-reach2"), CC.variant("denoise-reach2"), CC.other("denoise-reach2")):
        chains, stats = r.reach["chains"], r.reach["stats"]
        assert len(chains) == 6 and all(c[1] > 0 for c in chains), "every two-link chain has vectors that leave"
        assert [c[2] > 0 for c in chains] == [True, True, False, False, True, True], "fwd2[0], fwd2[1], bwd2[1], bwd2[2] through NaN or Inf; fwd2[2], bwd2[0] not"
        assert all(v > 0 for v in stats[2][1:5]) and all(stats[f][3] == stats[f][4] == 0 for f in (0, 4))
        assert [sum(v > 0 for v in s[1:5]) for s in stats] == [2, 3, 4, 3, 2]
        # the rings follow the pan: the neighbours get weight, and every frame changes
        assert all(s[7] > 0 and s[6] > 0 for s in stats) and all(r.want["frames"][f].tobytes() != r.frames[f].tobytes() for f in range(5))
        dead = np.isnan(r.want["fwd2"]).sum() + np.isnan(r.want["bwd2"]).sum()
        assert dead == 2 * sum(c[1] + c[2] for c in chains)
    assert CC.recipe("denoise-reach2").channels == 1 and CC.other("denoise-reach2").channels == 3
    a, b = CC.chain("denoise-reach2")
    assert (a.wc, b.wc) == (256, 37) and a.weights.tolist() == CC.TR.weights_for(10.0).tolist() and b.weights.tolist() == CC.TC.tables()["random"].tolist()
    CC.same(a.want["frames"], CC.recipe("denoise-reach2").want["frames"], "the chain's first call is the row")


def test_the_denoise_launch_is_the_engines_order_of_neighbours(monkeypatch):
    r = CC.recipe("denoise-reach2")
    (chain, filt), outs, ins = _recorded(monkeypatch, r)
    N, w, h, _ = CC.DENOISE
    planes, (fwd, bwd), field = ins[:N], ins[N:], 8 * w * h
    assert chain["n"] == 6 and filt["n"] == N
    for j, (ring, out) in enumerate(((fwd, outs["fwd2"]), (bwd, outs["bwd2"]))):
        for p in range(3):
            d = chain["descs"][3 * j + p]
            assert (d.d_link[0], d.d_link[1], d.n_links, d.d_dst) == (ring.ptr + p * field, ring.ptr + (p + 1) * field, 2, out.slot(p))
            assert d.d_mask is None and d.d_stats is None
    for f, d in enumerate(filt["descs"]):
        want = [(g, at) for g, at in ((f - 1, bwd.ptr + (N - 1 - f) * field), (f + 1, fwd.ptr + f * field), (f - 2, outs["bwd2"].slot(N - 1 - f)), (f + 2, outs["fwd2"].slot(f)))
                if 0 <= g < N]
        assert d.n_neighbours == len(want) and d.d_centre == planes[f].ptr and d.d_dst == outs["frames"].slot(f) and d.d_stats == outs["stats"].slot(f)
        assert [(d.neighbour[k].d_plane, d.neighbour[k].d_field) for k in range(len(want))] == [(planes[g].ptr, at) for g, at in want]
