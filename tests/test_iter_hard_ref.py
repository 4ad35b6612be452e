"""The oracle alone on the hard frames of tests/iter_hard.py (no GPU): the determinant guard of the iteration restatement
(oracle/ofx_oracle.c, orc_lk_iter_level_guard) against a NumPy restatement of include/ofx.h's definition, and the census -- every
case tests/test_gpu_iter_hard.py compares with the oracle really drives the warp into its "no warp" branch, its four clamps, the
last column and row, and puts non-finite flows next to the tile seam.  These are conditions on the test inputs, not measurements:
a case that misses one gets another seed or block position.

What the oracle measured on the cases as they stand (the smallest count over a case's pairs; "seam": non-finite pixels within R + 1
columns of the tile seam, "-" where the level is narrower than a tile; run with -s for every pair):

case                      lvl no_warp  sx<0 sx>w-1  sy<0 sy>h-1 lastcol lastrow  seam
A-win3                      0   3720     70     67    595    337    151    822   216
A-win5                      0   3344     39     52    348    266    123    757   272
A-win7                      0   3008     43     49    296    245    117    741   320
A-win9                      0   2688     56     27    326    216    114    706   360
A-win11                     0   2384     53     48    368    218    128    696   392
A-win13                     0   2096     64     56    395    218    138    721   416
A-win15                     0   1824     65     62    403    245    148    714   432
A-win17                     0   1628     72     86    267    267    176    756   440
A-win19                     0   1440     73     90    352    296    184    758   440
A-win21                     0   1260     75     94    396    294    192    777   432
A-win23                     0   1088     75     98    400    311    176    770   416
A2-win11                    0  23060     73     69    372    361    200   1335  1768
A2-win11                    1   3882     34     49    410    254    129    723   378
A2-win13                    0  21898     66     77    319    358    206   1399  1980
A2-win13                    1   3420     40     55    441    263    137    770   400
A2-win17                    0  19670     50    105    337    509    248   1476  2356
A2-win17                    1   2604     56     90    435    146    180    614   420
A2-win19                    0  18604     50    115    353    578    230   1497  2520
A2-win19                    1   2242     54     94    446    154    188    615   418
A2-win21                    0  17570    136     74     31    527    219   1455  2668
A2-win21                    1   1904     53     98    456    147    196    619   408
A2-win23                    0  16568    150     75     16    522    223   1448  2800
A2-win23                    1   1590     53    102    458    155    202    635   390
C-win9-w231-it4-B1          0  19806     62     64    540    257    185   1227  1287
C-win9-w231-it4-B1          1   3477     48     44    490    154    125    653   213
C-win9-w233-it5-B2          0  26408     85     93    789    532    254   1721  1716
C-win9-w233-it5-B2          1   4636     37     66    756    152    174    824   284
C-win9-w465-it4-B2          0  29592     71     49   1337    680    220   2678  1287
C-win9-w465-it4-B2          1   5424     32     60   1106    368    161   1455   528
C-win9-w465-it5-B1          0  39456     98    147   1806    962    415   3568  1716
C-win9-w465-it5-B1          1   7232     63     80   1449    496    214   1946   704
C-win3-w249-it5-B1          0  30608    414    364   2478   1330    502   2577   840
C-win3-w249-it5-B1          1   6412     50     90    475    342    172   1090   212
C-win5-w241-it4-B2          0  21882     94     21    819    344    127   1275   861
C-win5-w241-it4-B2          1   4320     32     20    333    118    102    623   189
C-win7-w241-it5-B2          0  27776    152     48    913    410    206   1584  1440
C-win7-w241-it5-B2          1   5172     37     60    500    130    154    822   276
C-win9-w233-it5-B1-packed   0  26408     85    103    789    586    259   1867  1716
C-win9-w233-it5-B1-packed   1   4636     44     68    756    270    176    943   284
C-win11-w241-it4-B1         0  18804     57     72    556    332    192   1330  1482
C-win11-w241-it4-B1         1   3087     35     54    614    188    143    740   207
C-win15-w241-it5-B2         0  22496     62    120    559    262    304   1608  2448
C-win15-w241-it5-B2         1   3124     55     72    904     98    216    862   212
D-3level                    0  29460    575    740   1510    357   1087    858  2024
D-3level                    1   4944     16    113    529    320    263    471     -
D-3level                    2    424     48     65    295    183    218    651     -
T3 of tests/lk_instances.py (the tick that also warps, two iterations, one column past a tile at level 1; B = 2 at the even radii):
C-win3-w249-it2-B1          0   7652     28     24    332    137     59    468   210
C-win3-w249-it2-B1          1   1603     10     13    106     65     33    233    53
C-win5-w241-it2-B2          0   7294     27      6    250     94     40    418   287
C-win5-w241-it2-B2          1   1440     10      7    105     38     35    207    63
C-win7-w241-it2-B1          0   6944     23     18    212    126     52    442   360
C-win7-w241-it2-B1          1   1293     10     16    124     71     40    245    69
C-win9-w233-it2-B2          0   6602     14     21    164    108     58    419   429
C-win9-w233-it2-B2          1   1159     10     16    194     40     43    209    71
C-win11-w241-it2-B1         0   6268     17     24    177    110     64    447   494
C-win11-w241-it2-B1         1   1029     14     18    204     64     47    250    69
C-win13-w241-it2-B2         0   5942     16     27    136     65     70    404   555
C-win13-w241-it2-B2         1    903     13     17    211     26     50    215    63
C-win15-w241-it2-B1         0   5624     18     30    135     86     76    432   612
C-win15-w241-it2-B1         1    781     14     19    230     70     55    262    53
C-win17-w233-it2-B2         0   5344     18     31    154     86     80    416   665
C-win17-w233-it2-B2         1    663     15     19    217     20     58    208    39
C-win19-w233-it2-B1         0   5068     18     32    158    121     84    464   714
C-win19-w233-it2-B1         1    549     17     21    224     65     63    282    21
C-win21-w233-it2-B2         0   4796     20     33    156     79     88    411   759
C-win21-w233-it2-B2         1    450     18     21    228     24     64    229    10
C-win23-w233-it2-B1         0   4528     21     34    147    150     92    484   800
C-win23-w233-it2-B1         1    369     18     23    228     85     65    281     9
(with B = 2 at the odd radii instead, pair 4 of window 23 has no tap clamped at sx < 0 on level 0: the batch sizes are the
other way round.)  Every pair of T3 and of T0 (the plain tick, one iteration, lk_float and compat_cpu, windows up to 25x25) has
non-finite flows at both levels.
guarded share of level 0 (min_det 5e9): A-win9 0.102, A-win15 0.060, C-win9-w233-it5-B2 0.242-0.244, C-win5-w241-it4-B2 0.444-0.455, D-3level 0.134-0.135
D-3level, both pairs: pixel 0 of levels 1 and 2 guarded, (nan, nan) unguarded; the shifted level-0 next image differs from the
unguarded run's in 41872..41881 of 63104 pixels
values under lk_solve.h's exception: A-win3 1 of 66732, A-win9 0 of 64588, A-win15 0 of 64588, A-win23 0 of 62444, C-win9-w233-it5-B2 0 of 1230240, C-win5-w241-it4-B2 1 of 954360
... A-win5 1 of 66732, and 0 for A-win7, 11, 13, 17, 19 and 21; T3: C-win3-w249-it2-B1 2 of 164340 (1.2e-5), 0 for the windows 5x5 .. 23x23 (153780 ..
318120 values each)
"""
import numpy as np
import pytest

from cuda_optical_flow_2_amd import synth
from conftest import assert_same
import iter_hard as ih
import lk_instances as li


def _ids(cases):
    return [c.id for c in cases]


def test_guard_off_is_the_unguarded_restatement(oracle, golden):
    """min_det = 0 keeps the bits the restatement gave before it had a guard.  orc_lk_iter_level is now the guarded function called
    with 0, so comparing the two would compare a function with itself: tests/golden/iter_hard_unguarded.npz holds a hard pair
    (hard_pair(130, 66, seam_x=60)) and what orc_lk_iter_level (9x9, 4 iterations) and flow_pair_iter (2 levels, 3 iterations) of
    the commit before the guard returned for it, NaN included."""
    g = golden("iter_hard_unguarded")
    p, n = g["prev"], g["next"]
    assert np.isnan(g["level_flow"]).any()
    for min_det in ((), (0.0,)):
        got, got_first = oracle.lk_iter_level(p, n, 9, 4, *min_det)
        assert_same(got.view(np.uint32), g["level_flow"].view(np.uint32), f"accumulated flow, min_det {min_det}")
        assert_same(got_first.view(np.uint32), g["level_first"].view(np.uint32), f"first iteration, min_det {min_det}")
        pyr = oracle.flow_pair_iter(p, n, 2, 9, 3, *min_det)
        for k in range(2):
            assert_same(pyr[k].view(np.uint32), g[f"pair_flow{k}"].view(np.uint32), f"pair, level {k}, min_det {min_det}")
    # the fixture's frames are still what hard_pair makes (the other tests of this file run on its like)
    hp, hn = ih.hard_pair(130, 66, seam_x=60)
    assert_same(hp, p, "hard_pair, prev")
    assert_same(hn, n, "hard_pair, next")


def test_guard_equals_its_definition(oracle):
    """include/ofx.h (ofx_lk_desc.min_det) / solve_guard of csrc/lk_solve.h, restated with NumPy on the oracle's pieces: after the
    solve of every iteration, det = Sxx Syy - Sxy^2 of the float sums in double, rounded once; !((float)det >= min_det) -> (0, 0)."""
    w, h, win, iters = 131, 67, 9, 3
    p, n = ih.hard_pair(w, h, seam_x=60)
    flow = None
    for it in range(iters):
        wimg = n if it == 0 else oracle.warp_bilinear_u8(n, flow)
        delta = oracle.lk_iter_level(p, wimg, win, 1)[0]
        s = oracle.level_planes(synth.to_3ch(p), synth.to_3ch(wimg), win, 1, exact_sums=True)[3]
        det = (s[0] * s[1] - s[2] * s[2]).astype(np.float32)
        low = ~(det >= np.float32(ih.MIN_DET))
        delta[low] = 0.0
        with np.errstate(invalid="ignore", over="ignore"):
            flow = delta if it == 0 else flow + delta
        if it == 0:
            first = flow.copy()
    got, got_first = oracle.lk_iter_level(p, n, win, iters, min_det=ih.MIN_DET)
    assert 0.01 < low.mean() < 0.99
    assert_same(got_first.view(np.uint32), first.view(np.uint32), "guarded first iteration")
    assert_same(got.view(np.uint32), flow.view(np.uint32), "guarded accumulated flow")
    assert_same(low, ih.guarded_mask(oracle, p, win, ih.MIN_DET), "guarded_mask")


def test_guarded_flat_block_is_exactly_zero(oracle):
    w, h, win = 131, 67, 9
    p, n = ih.hard_pair(w, h, seam_x=60)
    plain = oracle.lk_iter_level(p, n, win, 3)[0]
    guarded = oracle.lk_iter_level(p, n, win, 3, min_det=ih.MIN_DET)[0]
    y, x = h // 3 + 20, 60
    assert (p[y - 6: y + 7, x - 6: x + 7] == 77).all()
    assert np.isnan(plain[y, x]).all(), "the unguarded solve of a flat window is 0 / 0"
    assert (guarded[y, x].view(np.uint32) == 0).all(), "guarded: exactly (+0, +0)"
    nan = np.isnan(plain).any(axis=-1)
    assert (guarded[nan] == 0).all(), "every 0 / 0 pixel has det == 0 and is guarded"


def test_warp_census_counts_what_the_warp_does(oracle):
    """warp_census against hand-made flows: one pixel per branch"""
    w, h = 8, 6
    s = float(oracle.ITER_SCALE)
    f = np.zeros((h, w, 2), np.float32)
    f[0, 0] = (np.nan, 0)
    f[0, 1] = (0, np.inf)
    f[1, 1] = (-1e30, 0)            # beyond 1e9: no warp
    f[2, 2] = (-3 / s - 1, 0)       # sx < 0
    f[2, 3] = (5 / s + 1, 0)        # sx > w - 1
    f[3, 3] = (0, -4 / s - 1)       # sy < 0
    f[3, 4] = (0, 3 / s + 1)        # sy > h - 1
    c = ih.warp_census(f, w, h, s)
    assert (c["no_warp"], c["sx_lo"], c["sx_hi"], c["sy_lo"], c["sy_hi"]) == (3, 1, 1, 1, 1)
    # taps in the last column: columns w - 2 and w - 1 at zero flow (less the no-warp ones: none there), and the clamped pixel
    assert c["last_col"] == 2 * h + 1 and c["last_row"] == 2 * w + 1


CENSUS_CASES = ih.A_CASES + ih.C_CASES + [ih.D_CASES[-1]] + li.T3_CASES


@pytest.fixture(scope="module")
def report():
    rows = []
    yield rows
    if rows:
        print("\ncase                         pair lvl  no_warp  sx<0 sx>w-1  sy<0 sy>h-1 lastcol lastrow  seam")
        for r in rows:
            print(r)


@pytest.mark.parametrize("case", CENSUS_CASES, ids=_ids(CENSUS_CASES))
def test_census_of_the_unguarded_cases(oracle, report, case):
    """On the flow that enters each warp (after 1 .. iters - 1 iterations), summed over the iterations of a level, for every pair
    and every level at least 16 pixels wide and high: "no warp", each of the four clamps, a tap in the last column and in the last
    row at least once, and a non-finite pixel within R + 1 columns of the tile seam (on the levels wide enough to have that
    column).  The chain's last flow is what the GPU tests compare with: flow_pair_iter's."""
    frames = ih.case_frames(case)
    for pair in range(1, len(frames)):
        chain = ih.oracle_chain(oracle, frames[pair - 1], frames[pair], case.levels, case.win, case.iters)
        if case in li.T3_CASES:     # what tests/test_gpu_lk_instances.py compares: non-finite flows at both levels of every pair
            assert all(not np.isfinite(lv["flows"][-1]).all() for lv in chain), f"{case.id} pair {pair}: a level without non-finite flows"
        if pair == 1:
            for k, want in enumerate(oracle.flow_pair_iter(frames[0], frames[1], case.levels, case.win, case.iters)):
                assert_same(chain[k]["flows"][-1], want, f"{case.id}: the chain ends in flow_pair_iter's level {k}")
        for k, lv in enumerate(chain):
            hk, wk = lv["prev"].shape
            if wk < 16 or hk < 16:
                continue
            c = ih.level_census(oracle, lv, case.win, ih.level_seam(case, k))
            report.append(f"{case.id:28s} {pair:4d} {k:3d} " + " ".join(f"{c[key]:7d}" for key in ih.CENSUS_KEYS) + f" {c['seam']}")
            for key in ih.CENSUS_KEYS:
                assert c[key] >= 1, f"{case.id} pair {pair} level {k}: {key} = 0 ({c})"
            assert c["seam"] is None or c["seam"] >= 1, f"{case.id} pair {pair} level {k}: no non-finite flow at the seam ({c})"
            assert k != case.level or c["seam"] is not None, f"{case.id}: the level under test has no seam column"


@pytest.mark.parametrize("case", ih.D_CASES, ids=_ids(ih.D_CASES))
def test_census_of_the_guarded_cases(oracle, report, case):
    """With the guard on: more than 1 % of level 0 guarded and more than 1 % not, on every pair.  The three-level case (black
    top left corner): pixel 0 of every coarse level is guarded and its unguarded first-iteration flow is not (0, 0), so the shift
    vectors -- and with them the next image of the levels below -- differ between the guarded and the unguarded run."""
    frames = ih.case_frames(case)
    for pair in range(1, len(frames)):
        low = ih.guarded_mask(oracle, oracle.gauss_pyramid(synth.to_3ch(frames[pair - 1]), 1)[0][:, :, 0], case.win, ih.MIN_DET)
        share = float(low.mean())
        report.append(f"{case.id:28s} {pair:4d}   0  guarded share {share:.4f}")
        assert 0.01 < share < 0.99, f"{case.id} pair {pair}: guarded share {share}"
        chain = ih.oracle_chain(oracle, frames[pair - 1], frames[pair], case.levels, case.win, case.iters, ih.MIN_DET)
        got0 = chain[0]["flows"][0]
        assert (got0[low] == 0).all() and np.isfinite(got0).all(), f"{case.id} pair {pair}: guarded first iteration"
        if case.corner:
            # the guarded pixel 0 of every coarse level feeds the shift: guarded it is (0, 0), no shift; unguarded it is not (NaN:
            # a shift out of the image), so the levels below get another next image than without the guard
            plain = ih.oracle_chain(oracle, frames[pair - 1], frames[pair], case.levels, case.win, 1)
            for k in range(1, case.levels):
                assert ih.guarded_mask(oracle, chain[k]["prev"], case.win, ih.MIN_DET)[0, 0], f"{case.id} pair {pair} level {k}: pixel 0 is not guarded"
                assert (chain[k]["flows"][0][0, 0].view(np.uint32) == 0).all(), f"{case.id} pair {pair} level {k}: guarded pixel 0"
                assert not (plain[k]["flows"][0][0, 0] == 0).all(), f"{case.id} pair {pair} level {k}: unguarded pixel 0 is (0, 0) too"
                report.append(f"{case.id:28s} {pair:4d} {k:3d}  pixel 0 guarded; unguarded {plain[k]['flows'][0][0, 0].tolist()}")
            differ = int((chain[0]["next"] != plain[0]["next"]).sum())
            report.append(f"{case.id:28s} {pair:4d}   0  shifted next differs from the unguarded run's in {differ} pixels")
            assert differ > 0, f"{case.id} pair {pair}: the guard does not change the shift"


@pytest.mark.parametrize("win", range(3, 26, 2))
def test_every_pair_of_the_plain_tick_cases_has_non_finite_flows(oracle, win):
    """T0 of tests/lk_instances.py (one iteration, lk_float up to 23x23, compat_cpu up to 25x25; lk_float_fast is compared with
    lk_float's oracle): every pair, both levels -- in compat_cpu too.  The four pairs of B = 2 include the two of B = 1."""
    cases = [t for t in li.T0_CASES if t.case.win == win]
    assert {(t.mode, t.deep) for t in cases} == {(m, d) for m in (("lk_float", "compat_cpu", "lk_float_fast") if win <= 23 else ("compat_cpu",)) for d in (-1, 1)}
    assert {t.case.B for t in cases} == {1, 2} and len({(t.case.w, t.case.h, t.case.levels) for t in cases}) == 1
    c = max((t.case for t in cases), key=lambda c: c.B)
    frames = ih.case_frames(c)
    for mode in sorted({"lk_float" if t.mode == "lk_float_fast" else t.mode for t in cases}):
        for pair in range(1, len(frames)):
            flows = oracle.flow_pair(synth.to_3ch(frames[pair - 1]), synth.to_3ch(frames[pair]), c.levels, win, mode, exact_sums=True)[0]
            for k in range(c.levels):
                assert not np.isfinite(flows[k]).all(), f"window {win} {mode}: pair {pair} level {k} is finite throughout"


def _tap_rows_outside(orc, flow, h, rows, buf):
    """the pixels of rows [rows) whose warp (orc_warp_bilinear_u8's arithmetic, as iter_hard.warp_census) takes a tap from a row
    outside [buf) of a level of h rows: what a row window's launch reports in its status word (csrc/lk_body.h, LkArgs::warp_status)"""
    s = np.float32(orc.ITER_SCALE)
    yy = np.arange(h, dtype=np.float32)[:, None]
    big = np.float32(1e9)
    with np.errstate(invalid="ignore", over="ignore"):
        sx, sy = s * flow[..., 0], yy + s * flow[..., 1]
        warped = (sx >= -big) & (sx <= big) & (sy >= -big) & (sy <= big)      # (sx without its column: |x| is far below 1e9)
        cy = np.clip(np.where(warped, sy, 0), 0, np.float32(h - 1))
    y0 = cy.astype(np.int64)
    y1 = np.minimum(y0 + 1, h - 1)
    return int((warped & ((y0 < buf[0]) | (y1 >= buf[1])))[rows[0]: rows[1]].sum())


@pytest.mark.parametrize("c", li.T5_CASES, ids=_ids(li.T5_CASES))
def test_row_window_cases_stay_inside_their_rows(oracle, c):
    """T5 of tests/lk_instances.py asserts a status word of 0 on every rank.  On the oracle's chain of every pair: the flow that
    enters the warp of iteration j + 1 takes no tap from a row outside a rank's buffer, on the rows that rank warps (its own
    rows and (radius + 1) * (iters - j) more either side: csrc/session_stream.cpp, iter_passes), and pixel 0 of level 1 -- the
    shift vector of level 0 -- is finite and small against the margin of 8 rows."""
    frames = li.rows_frames(c)
    reach = (c.win >> 1) + 1
    for pair in range(1, len(frames)):
        chain = ih.oracle_chain(oracle, frames[pair - 1], frames[pair], c.levels, c.win, c.iters)
        corner = chain[c.levels - 1]["flows"][0][0, 0]
        assert np.isfinite(corner).all() and (np.abs(corner) <= 2).all(), f"{c.id} pair {pair}: pixel 0 of level {c.levels - 1} is {corner.tolist()}"
        for k, lv in enumerate(chain):
            for j, f in enumerate(lv["flows"][:-1], 1):
                for pl in li.shard_plans(c):
                    ext = reach * (c.iters - j)
                    rows = (max(pl.own[k][0] - ext, pl.buf[k][0]), min(pl.own[k][1] + ext, pl.buf[k][1]))
                    n = _tap_rows_outside(oracle, f, c.h >> k, rows, pl.buf[k])
                    assert n == 0, f"{c.id} pair {pair} level {k}, the warp of iteration {j + 1}: {n} pixels of rank {pl.rank} reach beyond its rows"


FAST_CASES = ih.E_CASES + li.T3_CASES     # what goes through iter_hard.check_fast_step


@pytest.mark.parametrize("case", FAST_CASES, ids=_ids(FAST_CASES))
def test_exempt_share_of_the_fast_cases(oracle, report, case):
    """Along the oracle's own chain: the pixel-steps that csrc/lk_solve.h's exception covers (iter_hard.fast_exempt) are at most
    1e-3 of a case's pixel-steps -- the step-by-step comparison of lk_float_fast is a 1-ulp test, not a test of the exception."""
    frames = ih.case_frames(case)
    steps = exempt = 0
    for pair in range(1, len(frames)):
        for lv in ih.oracle_chain(oracle, frames[pair - 1], frames[pair], case.levels, case.win, case.iters):
            for f in lv["flows"][:-1]:
                ex, _ = ih.fast_exempt(oracle, lv["prev"], oracle.warp_bilinear_u8(lv["next"], f), case.win)
                steps += ex.size
                exempt += int(ex.sum())
    report.append(f"{case.id:28s} exempt {exempt} of {steps} pixel-steps ({exempt / steps:.2e})")
    assert exempt <= 1e-3 * steps, f"{case.id}: {exempt} of {steps} pixel-steps exempt"
