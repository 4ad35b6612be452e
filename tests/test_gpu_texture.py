"""GPU: texture strength and feature selection -- ofx_texture_features, ofx_compact_features, engine.texture_strength,
engine.good_features and engine.video_tracks_auto -- against tests/texture_ref.py.  Every comparison is exact, floats by their
bits.  Outputs sit in buffers of 0x5A, inputs in larger buffers whose surroundings differ between runs, so that a tap outside an
input, or a store outside an output, shows."""
import ctypes as C
import functools

import numpy as np
import pytest

import texture_ref as T
from test_gpu_interp import AROUND_P, FILL, Guarded, Plane, same

pytestmark = pytest.mark.gpu

OFX_E_INVALID = 1
NB = 16                                                   # OFX_STREAM_MAX_BATCH
STRIP, tile_out = T.STRIP, T.tile_out                     # kStrip and kTile - 2R of csrc/texture.hip: a block's output rows and columns


def shapes(win):
    """(w, h): the tiny and odd ones, two blocks across and two down, and one column more than a tile and one row more than a strip"""
    return [(1, 1), (2, 3), (5, 4), (63, 7), (65, 9), (262, 74), (263, 75), (tile_out(win) + 1, STRIP + 1)]


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cuda_optical_flow_2_amd import engine

    return engine


@pytest.fixture(scope="module")
def orc():
    import oracle

    oracle.build()
    return oracle.Oracle()


@functools.lru_cache(maxsize=None)
def _shared(kind, w, h):
    a = T.make_input(kind, w, h)
    a.setflags(write=False)
    return a


def _img(kind, w, h):
    """a copy the callee may do with what it likes"""
    return np.array(_shared(kind, w, h))


_WANT = {}


def want_strength(orc, kind, w, h, win):
    """the referee's strength, computed once and shared"""
    key = (kind, w, h, win)
    if key not in _WANT:
        r = T.strength(orc, _shared(kind, w, h), win)
        r.setflags(write=False)
        _WANT[key] = r
    return _WANT[key]


def pad4(w):
    return (w + 3) & ~3


class Item:
    """one item of a launch on guarded buffers: the plane inside a larger buffer of `around`, every output inside 0x5A"""

    def __init__(self, img, pitch, around, sp, cell=None, border=0, thr=0.0, stats=True, lead=8):
        h, w = img.shape
        self.w, self.h, self.sp, self.cell = w, h, sp, cell
        self.plane = Plane(img, pitch, lead, around)
        self.strength = Guarded(np.float32, 1, h, w, sp, 4)
        self.cells = self.cs = self.stats = None
        if cell is not None:
            self.ncx, self.ncy = T.grid(w, h, cell)
            self.cells = Guarded(np.int32, 1, self.ncy, 2 * self.ncx, 2 * self.ncx, 2)
            self.cs = Guarded(np.float32, 1, self.ncy, self.ncx, self.ncx, 3)
            if stats:
                self.stats = Guarded(np.int64, 1, 1, 4, 4, 1)
        self.border, self.thr = border, thr

    def desc(self, lib):
        return lib.TextureDesc(self.plane.ptr, self.plane.pitch, self.w, self.h, self.strength.ptr, self.sp,
                               self.cells.ptr if self.cells else None, self.cs.ptr if self.cs else None, self.stats.ptr if self.stats else None,
                               self.cell or 0, self.border, self.thr)

    def check(self, orc, want_r, what):
        got, clean = self.strength.host()
        assert clean, f"{what}: a store outside the strength plane (pad floats included)"
        same(got[0], want_r, f"{what}: strength")
        if self.cells:
            cells, cs, stats = T.select(want_r, self.cell, self.border, self.thr)
            got, clean = self.cells.host()
            assert clean, f"{what}: a store outside cells"
            same(got[0].reshape(self.ncy, self.ncx, 2), cells, f"{what}: cells")
            got, clean = self.cs.host()
            assert clean, f"{what}: a store outside cell_strength"
            same(got[0], cs, f"{what}: cell_strength")
            if self.stats:
                got, clean = self.stats.host()
                assert clean and got.reshape(4).tolist() == stats.tolist(), f"{what}: stats {got.reshape(4).tolist()} vs {stats.tolist()}"


def launch(eng, items, win):
    import torch

    lib = eng._lib
    d = (lib.TextureDesc * len(items))(*[it.desc(lib) for it in items])
    eng.check(lib.load().ofx_texture_features(d, len(items), win, eng._stream_ptr()), "ofx_texture_features")
    torch.cuda.synchronize()


# ---- 1. strength ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("win", T.WINDOWS)
def test_strength_equals_the_referee(eng, orc, win):
    """every shape x every input, sixteen items of mixed sizes per launch; each item once with the tight pitch (w rounded up to 4)
    and strength_pitch w and once with larger ones, the surroundings of the planes differing between the two runs.  The noise and
    the checkerboard are what pin the square root's rounding: their sums are large and all different."""
    cases = [(kind, w, h) for (w, h) in shapes(win) for kind in T.INPUTS]
    for run in (0, 1):
        for i0 in range(0, len(cases), NB):
            batch = cases[i0:i0 + NB]
            items = []
            for j, (kind, w, h) in enumerate(batch):
                loose = (j + run) & 1
                items.append(Item(_img(kind, w, h), pad4(w) + 8 * loose, AROUND_P[run], w + 3 * loose, lead=8 + 4 * loose))
            launch(eng, items, win)
            for it, (kind, w, h) in zip(items, batch):
                it.check(orc, want_strength(orc, kind, w, h, win), f"win {win} run {run} {kind} {w}x{h}")


@pytest.mark.parametrize("win", [w for w in T.ALL_WINDOWS if w not in T.WINDOWS])
def test_strength_of_every_other_instance_equals_the_referee(eng, orc, win):
    """the eight instances of strength_kernel<R> that T.WINDOWS leaves out, each on the fewest shapes and inputs that tell its
    constants -- the ring's 2R + 1 rows and its wrap, the phases of the march, OUT_W = 256 - 2R and with it the tile seams: twelve
    items of mixed sizes in one launch, once with tight pitches and once with larger ones, as above.  tests/test_texture_ref.py
    shows that on the two larger shapes the referee's plane at a window is not its plane at a neighbouring one."""
    cases = [(kind, w, h) for (w, h) in T.instance_shapes(win) for kind in T.INSTANCE_INPUTS]
    assert len(cases) <= NB
    for run in (0, 1):
        items = []
        for j, (kind, w, h) in enumerate(cases):
            loose = (j + run) & 1
            items.append(Item(_img(kind, w, h), pad4(w) + 8 * loose, AROUND_P[run + 1], w + 3 * loose, lead=8 + 4 * loose))
        launch(eng, items, win)
        for it, (kind, w, h) in zip(items, cases):
            it.check(orc, want_strength(orc, kind, w, h, win), f"win {win} run {run} {kind} {w}x{h}")


@pytest.mark.parametrize("win", T.WINDOWS)
def test_strength_equals_the_chain_on_the_device(eng, win):
    """ofx_lk_level_sums(p, p) -- the definition's step 1 as the library itself writes it -- then steps 2 and 3 in NumPy"""
    for kind, w, h in (("noise", 263, 75), ("checker", tile_out(win) + 1, STRIP + 1), ("hard", 264, 80)):
        p = _img(kind, w, h)
        sums = eng.lk_level(p, p, win, "lk_float", want_sums=True)
        assert sums.dtype == np.int32 and sums.shape == (5, h, w)
        same(eng.texture_strength(p, win), T.strength_of_sums(sums[0], sums[1], sums[2]), f"win {win} {kind} {w}x{h}")


# ---- 2. selection ---------------------------------------------------------------------------------------------------------------

SELECT_FIELDS = [("hard", 264, 80), ("noise", 263, 75), ("checker", 66, 50), ("const", 70, 41), ("tiled", 96, 40), ("smooth", 65, 9), ("noise", 5, 4), ("noise", 2, 3),
                 ("noise", 1, 1)]


@pytest.mark.parametrize("cell", [4, 16, 37])
def test_selection_equals_the_referee(eng, orc, cell):
    """cells, strengths and stats, with the default border, without one (the plateaus along a constant image's edge and of the
    checkerboard meet the plateau rule, the repeated maxima of the tiled patch the tie rule) and with a threshold; fields smaller than a cell and
    smaller than twice the border are among them"""
    win = 9
    b = T.default_border(win)
    for run, (border, thr) in enumerate(((b, 0.0), (0, 0.0), (2, 3.0e5))):
        items = [Item(_img(kind, w, h), pad4(w) + 4 * (run & 1), AROUND_P[run], w + (run & 1), cell, border, thr) for (kind, w, h) in SELECT_FIELDS]
        launch(eng, items, win)
        for it, (kind, w, h) in zip(items, SELECT_FIELDS):
            it.check(orc, want_strength(orc, kind, w, h, win), f"cell {cell} border {border} thr {thr} {kind} {w}x{h}")


def test_selection_where_a_block_takes_several_groups(eng, orc):
    """csrc/texture.hip launches at most kSelectBlocks = 256 blocks per item and a block takes its groups (64 x 64 pixels at cell 4)
    in turn: 18 x 17 = 306 groups here, so 50 blocks take two, beside an item of one group in the same launch"""
    win, cell = 3, 4
    spec = [("smooth", 1090, 1028), ("noise", 40, 41)]
    assert -(-1090 // 64) * -(-1028 // 64) == 306 > 256
    items = [Item(_img(kind, w, h), pad4(w), 0x5A, w, cell, T.default_border(win)) for (kind, w, h) in spec]
    launch(eng, items, win)
    for it, (kind, w, h) in zip(items, spec):
        it.check(orc, want_strength(orc, kind, w, h, win), f"{kind} {w}x{h}")


def test_sixteen_items_of_different_sizes_and_cells_in_one_launch(eng, orc):
    win = 3
    sizes = [(1, 1), (2, 3), (5, 4), (63, 7), (65, 9), (262, 74), (263, 75), (tile_out(win) + 1, STRIP + 1), (31, 33), (64, 64), (100, 3), (3, 100),
             (17, 17), (128, 16), (40, 41), (257, 5)]
    cells = [4, 5, 7, 16, 37, 64, 100, 256, 8, 16, 4, 6, 17, 32, 13, 255]
    items = [Item(_img(T.INPUTS[i % 4], w, h), pad4(w), AROUND_P[i % 3], w, c, i % 3, 0.0 if i % 2 else 1000.0, stats=i % 5 != 4)
             for i, ((w, h), c) in enumerate(zip(sizes, cells))]
    launch(eng, items, win)
    for i, (it, (w, h)) in enumerate(zip(items, sizes)):
        it.check(orc, want_strength(orc, T.INPUTS[i % 4], w, h, win), f"item {i} {w}x{h} cell {cells[i]}")


def test_three_items_of_which_one_is_strength_only(eng, orc):
    win = 23
    spec = [("hard", 264, 80, 16), ("noise", 263, 75, None), ("checker", 66, 50, 37)]
    for order in (spec, spec[1:] + spec[:1]):
        items = [Item(_img(kind, w, h), pad4(w), 0x5A, w + 1, c, T.default_border(win)) for (kind, w, h, c) in order]
        launch(eng, items, win)
        for it, (kind, w, h, c) in zip(items, order):
            it.check(orc, want_strength(orc, kind, w, h, win), f"{kind} {w}x{h} cell {c}")


# ---- 3. compaction --------------------------------------------------------------------------------------------------------------

def test_compaction(eng, orc):
    """max_points below, equal to and above the occupied count; more cells than one pass of the block takes; no cell occupied"""
    import torch

    L = eng._lib.load()
    R = want_strength(orc, "hard", 264, 80, 9)
    for cell in (4, 16):
        cells, _, stats = T.select(R, cell, T.default_border(9), 0.0)
        n_cells, occupied = int(stats[0]), int(stats[1])
        assert occupied >= 3 and (cell != 4 or n_cells > 1024)
        d_cells = torch.from_numpy(cells).cuda()
        for max_points in (0, 1, occupied - 1, occupied, occupied + 1, n_cells + 7):
            pts = Guarded(np.float32, 1, 1, 2 * max(max_points, 1), 2 * max(max_points, 1), 2)
            cnt = Guarded(np.int32, 1, 1, 1, 1, 1)
            eng.check(L.ofx_compact_features(d_cells.data_ptr(), n_cells, max_points, pts.ptr, cnt.ptr, eng._stream_ptr()), "ofx_compact_features")
            torch.cuda.synchronize()
            want, occ = T.compact(cells, max_points)
            assert occ == occupied
            got_n, clean = cnt.host()
            assert clean and int(got_n.reshape(())) == min(occupied, max_points) == len(want)
            got, clean = pts.host()
            assert clean
            got = got.reshape(-1, 2)
            same(got[:len(want)], want, f"cell {cell} max_points {max_points}")
            assert (got[len(want):].view(np.uint8) == FILL).all(), f"cell {cell} max_points {max_points}: entries beyond the count were written"
    empty = torch.full((300, 2), -1, dtype=torch.int32, device="cuda")
    pts = Guarded(np.float32, 1, 1, 8, 8, 2)
    cnt = Guarded(np.int32, 1, 1, 1, 1, 1)
    eng.check(L.ofx_compact_features(empty.data_ptr(), 300, 4, pts.ptr, cnt.ptr, eng._stream_ptr()), "ofx_compact_features")
    torch.cuda.synchronize()
    assert int(cnt.host()[0].reshape(())) == 0 and (pts.host()[0].view(np.uint8) == FILL).all()


# ---- 4. the Python surface --------------------------------------------------------------------------------------------------------

def test_good_features_equals_the_referee(eng, orc):
    import torch

    f = _img("hard", 264, 80)
    for win, cell, border, thr, cap in ((9, 16, None, 0.0, None), (3, 4, 0, 0.0, None), (23, 37, None, 1.0e4, 5), (9, 16, 3, 0.0, 1000)):
        want_p, want_s = T.good_features(orc, f, win, cell, border, thr, cap)
        got_p, got_s = eng.good_features(f, win, cell, border, thr, cap)
        same(got_p, want_p, f"points win {win} cell {cell}")
        same(got_s, want_s, f"strengths win {win} cell {cell}")
        t = torch.from_numpy(np.array(f)).cuda()
        dev_p, dev_s = eng.good_features(t, win, cell, border, thr, cap)          # a tight CUDA tensor: read through a padded copy
        assert dev_p.is_cuda and dev_s.is_cuda
        same(dev_p.cpu().numpy(), want_p, "points of a CUDA tensor")
        same(dev_s.cpu().numpy(), want_s, "strengths of a CUDA tensor")
    same(eng.texture_strength(f, 9), want_strength(orc, "hard", 264, 80, 9), "texture_strength")
    padded = torch.zeros((80, 320), dtype=torch.uint8, device="cuda")
    padded[:, :264] = torch.from_numpy(np.array(f)).cuda()
    same(eng.texture_strength(padded[:, :264], 9).cpu().numpy(), want_strength(orc, "hard", 264, 80, 9), "texture_strength in place")
    flat = np.full((40, 40), 9, np.uint8)
    p, s = eng.good_features(flat, 9)
    assert p.shape == (0, 2) and s.shape == (0,) and p.dtype == np.float32


@pytest.mark.parametrize("level", [0, 1])
def test_video_tracks_auto_equals_video_tracks_fed_the_referees_points(eng, orc, level):
    import torch
    from cuda_optical_flow_2_amd import synth

    w, h, levels, win = 96, 64, 2, 9
    frames = np.stack([synth.smooth_pair(w, h, 1.5 * i, 0.75 * i)[1] for i in range(3)])
    clip = torch.from_numpy(frames).cuda()
    plane = frames[0] if level == 0 else np.ascontiguousarray(orc.gauss_pyramid(synth.to_3ch(frames[0]), levels)[level][:, :, 0])
    pts, strengths = T.good_features(orc, plane, win, 16)
    assert len(pts) >= 4
    want_pos, want_status = eng.video_tracks(clip, pts, levels, win, level=level)
    got_pos, got_status, got_s = eng.video_tracks_auto(clip, levels, win, 16, level)
    same(got_pos[0].cpu().numpy(), pts, "the seeds")
    same(got_pos.cpu().numpy(), want_pos.cpu().numpy(), "positions")
    same(got_status.cpu().numpy(), want_status.cpu().numpy(), "status")
    same(got_s.cpu().numpy(), strengths, "strengths")


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------

def test_a_refused_launch_enqueues_nothing(eng, orc):
    """live buffers: one bad item among good ones, and every output of every item still holds 0x5A afterwards"""
    import torch

    lib = eng._lib
    L = lib.load()

    def fresh():
        return [Item(_img("noise", 65, 9), 68, 0x00, 65, 16, 5), Item(_img("noise", 63, 7), 64, 0xFF, 66, None), Item(_img("smooth", 65, 9), 68, 0x5A, 65, 4, 0)]

    def spoil(i, **kw):
        items = fresh()
        d = (lib.TextureDesc * 3)(*[it.desc(lib) for it in items])
        for k, v in kw.items():
            setattr(d[i], k, v(getattr(d[i], k)) if callable(v) else v)
        return items, d

    cases = [(2, dict(cell=3), b"cell"), (0, dict(border=-1), b"border"), (2, dict(min_strength=float("nan")), b"min_strength"),
             (1, dict(pitch=66), b"pitch"), (1, dict(strength_pitch=62), b"strength_pitch"), (0, dict(d_plane=lambda p: p + 1), b"aligned"),
             (2, dict(d_strength=lambda p: p + 2), b"aligned"), (0, dict(d_cell_strength=None), b"go together"), (1, dict(d_stats=lambda p: 0x1000), b"d_stats without"),
             (2, dict(d_stats=lambda p: p + 4), b"aligned"), (1, dict(w=0), b"positive")]
    for i, kw, word in cases:
        items, d = spoil(i, **kw)
        rc = L.ofx_texture_features(d, 3, 9, eng._stream_ptr())
        msg = L.ofx_last_error()
        assert rc == OFX_E_INVALID and word in msg and b"item %d" % i in msg, (kw, rc, msg)
        torch.cuda.synchronize()
        for it in items:
            for g in (it.strength, it.cells, it.cs, it.stats):
                if g is not None:
                    assert (g.flat.cpu().numpy() == FILL).all(), f"{kw}: something was written"
    items, d = spoil(0)
    for win in (8, 25, 1):
        assert L.ofx_texture_features(d, 3, win, eng._stream_ptr()) == OFX_E_INVALID and b"window" in L.ofx_last_error()
    for n in (0, 17):
        assert L.ofx_texture_features(d, n, 9, eng._stream_ptr()) == OFX_E_INVALID and b"n = " in L.ofx_last_error()
    torch.cuda.synchronize()
    assert all((it.strength.flat.cpu().numpy() == FILL).all() for it in items)
    with pytest.raises(eng.OfxError):
        eng.good_features(_img("noise", 65, 9), 8)
    with pytest.raises(eng.OfxError):
        eng.good_features(_img("noise", 65, 9), 9, cell=3)
    with pytest.raises(eng.OfxError):
        eng.texture_strength(_img("noise", 65, 9), 25)
    launch(eng, items, 9)                                  # and with everything in place the same buffers run
    for it, (kind, w, h) in zip(items, (("noise", 65, 9), ("noise", 63, 7), ("smooth", 65, 9))):
        it.check(orc, want_strength(orc, kind, w, h, 9), f"after the refusals: {kind} {w}x{h}")
