"""CPU: the referee of texture strength and feature selection (tests/texture_ref.py) against what the definition (include/ofx.h,
"texture strength and feature selection") says in words.

The derivative taps outside the image are skipped, so the outermost ring of pixels of ANY image that is not black there has
derivatives, and a window that reaches that ring has strength: that is the definition (ofx_lk_level_sums' sums), and the reason
for the default border window // 2 + 1, the first at which no window of a candidate touches the ring.  "Everywhere" below
therefore means: everywhere for a black image, and everywhere inside that border for any other."""
import numpy as np
import pytest

import texture_ref as T


def _inside(R, b):
    return R[b:R.shape[0] - b, b:R.shape[1] - b]


@pytest.mark.parametrize("win", T.WINDOWS)
def test_a_constant_image_has_no_strength_and_no_candidate(oracle, win):
    b = T.default_border(win)
    black = T.strength(oracle, np.zeros((41, 70), np.uint8), win)
    assert black.dtype == np.float32 and not black.view(np.uint32).any()                 # +0 by the bits, everywhere
    R = T.strength(oracle, np.full((41, 70), 77, np.uint8), win)
    assert not _inside(R, b).view(np.uint32).any()
    assert R[0, 0] > 0 and (R >= 0).all()                                                # the image's corner is one: taps skipped
    for cell in (4, 16, 37):
        cells, cs, stats = T.select(R, cell, b, 0.0)
        ncx, ncy = T.grid(70, 41, cell)
        assert (cells == -1).all() and not cs.view(np.uint32).any()
        assert stats.tolist() == [ncx * ncy, 0, 0, (70 - 2 * b) * (41 - 2 * b)]
        assert not T.candidates(R, b, 0.0)[1].any()


@pytest.mark.parametrize("win", T.WINDOWS)
def test_a_single_vertical_step_edge_has_no_strength_and_yields_no_feature(oracle, win):
    """the aperture problem: Syy = Sxy = 0, so lambda = 0.5 * (Sxx - sqrt(Sxx^2)) = 0 exactly"""
    img = np.zeros((48, 64), np.uint8)
    img[:, 30:] = 200
    b = T.default_border(win)
    sxx, syy, sxy = T.exact_sums(oracle, img, win)
    assert _inside(sxx, b).max() > 0 and not _inside(syy, b).any() and not _inside(sxy, b).any()
    R = T.strength(oracle, img, win)
    assert not _inside(R, b).view(np.uint32).any()
    cells, cs, stats = T.select(R, 16, b, 0.0)
    assert (cells == -1).all() and stats[1] == 0 and stats[2] == 0 and stats[3] == (64 - 2 * b) * (48 - 2 * b)
    pts, occupied = T.compact(cells)
    assert pts.shape == (0, 2) and occupied == 0


@pytest.mark.parametrize("win", (3, 9))
def test_a_bright_rectangle_on_black_has_features_in_the_cells_of_its_corners(oracle, win):
    img = np.zeros((96, 128), np.uint8)
    x0, x1, y0, y1 = 24, 104, 24, 72                      # the rectangle [x0, x1) x [y0, y1): its corners lie in four cells of 16
    img[y0:y1, x0:x1] = 220
    R = T.strength(oracle, img, win)
    cells, cs, stats = T.select(R, 16, T.default_border(win), 0.0)
    occupied = {(cx, cy) for cy in range(cells.shape[0]) for cx in range(cells.shape[1]) if cells[cy, cx, 0] >= 0}
    r = win >> 1
    for (cx, cy) in ((x0, y0), (x1 - 1, y0), (x0, y1 - 1), (x1 - 1, y1 - 1)):
        near = [(x, y) for (x, y) in cells.reshape(-1, 2) if x >= 0 and abs(x - cx) <= r + 1 and abs(y - cy) <= r + 1]
        assert near, f"no feature within {r + 1} of the corner ({cx}, {cy})"
    # ... and nowhere else: along an edge, inside and outside the strength is 0
    for (x, y) in cells.reshape(-1, 2):
        if x >= 0:
            assert min(abs(x - x0), abs(x - (x1 - 1))) <= r + 1 and min(abs(y - y0), abs(y - (y1 - 1))) <= r + 1
    assert stats[1] == len(occupied) >= 4 and (cs[cells[..., 0] >= 0] > 0).all()


def test_of_a_plateau_the_first_pixel_in_raster_order_remains():
    R = np.zeros((12, 12), np.float32)
    R[4:6, 5:8] = 3.0                                     # six equal pixels
    R[9, 2] = R[9, 3] = 2.0                               # two equal pixels side by side
    R[2, 2], R[3, 3] = 1.0, 1.0                           # two equal pixels on a diagonal
    _, cand = T.candidates(R, 0, 0.0)
    assert sorted(map(tuple, np.argwhere(cand).tolist())) == [(2, 2), (4, 5), (9, 2)]
    R[5, 7] = np.nextafter(np.float32(3.0), np.float32(4.0))      # one pixel of the plateau a little larger: it remains, and so
    _, cand = T.candidates(R, 0, 0.0)                             # does (4, 5), which is no neighbour of it (the rule is local)
    assert sorted(map(tuple, np.argwhere(cand).tolist())) == [(2, 2), (4, 5), (5, 7), (9, 2)]
    R[4, 6] = R[5, 7]                                             # ... until a larger pixel is next to it
    _, cand = T.candidates(R, 0, 0.0)
    assert sorted(map(tuple, np.argwhere(cand).tolist())) == [(2, 2), (4, 6), (9, 2)]


def test_of_equal_candidates_in_a_cell_the_smallest_index_wins():
    R = np.zeros((16, 32), np.float32)
    R[10, 3] = R[2, 9] = R[2, 13] = 5.0                   # three separate equal maxima in cell (0, 0) of 16
    R[5, 20], R[12, 28] = 4.0, 6.0                        # cell (1, 0): the larger one wins wherever it lies
    cells, cs, stats = T.select(R, 16, 0, 0.0)
    assert cells.tolist() == [[[9, 2], [28, 12]]] and cs.tolist() == [[5.0, 6.0]]
    assert stats.tolist() == [2, 2, 5, 16 * 32 - 5]
    pts, occupied = T.compact(cells)
    assert pts.tolist() == [[9.0, 2.0], [28.0, 12.0]] and pts.dtype == np.float32 and occupied == 2
    assert T.compact(cells, 1)[0].tolist() == [[9.0, 2.0]] and T.compact(cells, 0)[0].shape == (0, 2)


def test_the_border_and_min_strength_with_its_strict_comparison():
    R = np.zeros((20, 20), np.float32)
    R[2, 2], R[3, 10], R[10, 16], R[17, 9] = 9.0, 8.0, 7.0, 6.0
    R[10, 10] = 5.0
    for b, want in ((0, 5), (2, 5), (3, 3), (4, 1), (10, 0), (11, 0), (40, 0)):
        inside, cand = T.candidates(R, b, 0.0)
        assert int(cand.sum()) == want and int(inside.sum()) == max(20 - 2 * b, 0) ** 2, b
    # a neighbour outside the border still suppresses: the border is a test of the pixel, not a crop of the plane
    R2 = R.copy()
    R2[9, 9] = 5.5                                         # next to (10, 10); with b = 10 .. nothing; with b = 4 both inside
    assert int(T.candidates(R2, 4, 0.0)[1].sum()) == 1 and T.candidates(R2, 4, 0.0)[1][9, 9]
    for thr, want in ((0.0, 5), (5.0, 4), (np.nextafter(np.float32(5.0), np.float32(0.0)), 5), (8.0, 1), (9.0, 0)):
        cells, cs, stats = T.select(R, 4, 0, thr)
        assert stats[2] == want == stats[1], thr          # (every maximum has a cell of 4 of its own)
        assert stats[3] == int((R <= np.float32(thr)).sum())
    assert T.select(R, 256, 0, 0.0)[0].tolist() == [[[2, 2]]]     # one cell for the whole plane: the largest


@pytest.mark.parametrize("win,grid_on_zero,zero_tenths,with_feature", [(3, 13, 163, 76), (9, 11, 123, 69), (23, 4, 50, 33)])
def test_the_census_of_the_hard_frame(oracle, win, grid_on_zero, zero_tenths, with_feature):
    """On hard_frames(264, 80, 2, seed=5)[0] -- flat blocks, stripes, noise -- no selected feature has strength 0, while 13 / 11 / 4
    of the 80 centres of the 16-pixel cells do at windows 3 / 9 / 23."""
    f = T.hard_frame()
    assert f.shape == (80, 264)
    R = T.strength(oracle, f, win)
    cells, cs, stats = T.select(R, 16, T.default_border(win), 0.0)
    gy, gx = np.mgrid[8:80:16, 8:264:16]
    assert gy.size == 80 and int((R[gy, gx] == 0).sum()) == grid_on_zero
    assert round(1000 * float((R == 0).mean())) == zero_tenths
    occ = cells[..., 0] >= 0
    assert cells.shape == (5, 17, 2) and int(occ.sum()) == with_feature == stats[1] and stats[0] == 85
    assert (cs[occ] > 0).all() and not cs[~occ].view(np.uint32).any()
    assert np.array_equal(cs[occ], R[cells[occ][:, 1], cells[occ][:, 0]])
    pts, strengths = T.good_features(oracle, f, win)
    assert len(pts) == with_feature and (strengths > 0).all() and np.array_equal(pts, cells[occ].astype(np.float32))


def test_a_checkerboard_at_window_23_stays_below_2_to_the_31(oracle):
    """0 / 255 squares of 2 x 2: every interior pixel has |Ix| = |Iy| = 510 or |Ix| + |Iy| = 1020; 529 of them"""
    sxx, syy, sxy = T.exact_sums(oracle, T.checkerboard(64, 48), 23)      # (asserts < 2^31 itself)
    top = max(int(np.abs(s).max()) for s in (sxx, syy, sxy))
    assert 2 ** 24 < top < 2 ** 31                        # ... and above float32's exact integers: the oracle's planes are rounded there
    R = T.strength(oracle, T.checkerboard(64, 48), 23)
    assert np.isfinite(R).all() and R.max() > 0


def test_the_strength_rounds_once_and_is_never_negative_zero():
    s = T.strength_of_sums([0, 5, 7, 2 ** 30, 3], [0, 5, 0, 2 ** 30, 3], [0, 5, 0, 2 ** 30 - 1, -3])
    assert s.dtype == np.float32 and not np.signbit(s).any() and not np.isnan(s).any()
    assert s[0] == 0 and s[1] == 0 and s[2] == 0 and s[4] == 0           # flat; Sxy^2 = Sxx Syy; one edge; the same with Sxy < 0
    assert s[3] == np.float32(0.5 * (2.0 ** 31 - np.sqrt(4.0 * float(2 ** 30 - 1) ** 2)))


@pytest.mark.parametrize("win", T.ALL_WINDOWS)
def test_no_window_has_its_neighbours_strength_on_the_instance_inputs(oracle, win):
    """tests/test_gpu_texture.py runs every instance of the strength kernel on T.instance_shapes x T.INSTANCE_INPUTS.  A launch that
    ran the instance of window W - 2 or W + 2 in W's place must not pass: on the two larger shapes the referee's planes of
    neighbouring windows differ, by the bits, in more than 0.99 of the pixels on the noise and on the checkerboard (measured: in every
    pixel) and in more than 0.75 on the hard frame (measured: 0.81 .. 0.95; its flat blocks have strength 0 at both).  The two
    small shapes are there for the clipping: every window covers the whole of 1 x 1, and from 9 on the whole of 5 x 4."""
    assert T.ALL_WINDOWS == (3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23) and set(T.WINDOWS) < set(T.ALL_WINDOWS)
    shapes = T.instance_shapes(win)
    assert shapes == [(256 - (win - 1) + 1, 65), (263, 75), (5, 4), (1, 1)]
    for (w, h) in shapes[:2]:
        for kind in T.INSTANCE_INPUTS:
            img = T.make_input(kind, w, h)
            R = T.strength(oracle, img, win)
            for other in (win - 2, win + 2):
                if other in T.ALL_WINDOWS:
                    share = float((R.view(np.uint32) != T.strength(oracle, img, other).view(np.uint32)).mean())
                    print(f"window {win} against {other}, {kind} {w}x{h}: {share:.4f} of the pixels differ")
                    assert share > (0.75 if kind == "hard" else 0.99), (win, other, kind, w, h, share)
