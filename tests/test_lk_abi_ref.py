"""CPU: the cases of tests/lk_abi_cases.py are what they claim, shown on the oracle alone -- the old flows of the accumulating cases
hold every special value, a warp case meets every branch of the oracle's warp, the determinant guard zeroes some pixels and not all,
the two row-window cases are the ones with and without a missing row, and the one restatement the cases carry (warp_rows) is the
oracle's warp on whole levels."""
import numpy as np

import iter_hard as ih
import lk_abi_cases as K

ALL_KINDS = {"nan", "+inf", "-inf", "1e30", "-0", "ordinary"}


def test_geometries_cover_every_pitch_lead_and_alignment():
    g = [K.geo(i) for i in range(9)]
    assert {(x.pitch, x.lead) for x in g} == {(p, l) for p in K.PITCH_KINDS for l in K.PLANE_LEADS}
    assert {x.flow_lead for x in g[:2]} == set(K.FLOW_LEADS)
    for w in (1, 2, 5, 37, 250, 259):
        assert K.pitch_of("tight", w) == (w + 3) & ~3 and K.pitch_of("tight+4", w) == K.pitch_of("tight", w) + 4
        assert K.pitch_of("wide", w) % 64 == 12 and all(K.pitch_of(k, w) % 4 == 0 and K.pitch_of(k, w) >= w for k in K.PITCH_KINDS)
    used = {(c.geo.pitch, c.geo.lead) for c in K.PLAIN}
    assert len(used) == 9 and {c.geo.flow_lead for c in K.PLAIN} == set(K.FLOW_LEADS)
    assert {c.uv for c in K.PLAIN} == set(K.UV_CASES) and any(c.rows for c in K.PLAIN)
    for c in K.PLAIN:
        if c.rows:
            row0, rows, y0, y1, f0 = c.rows
            assert row0 > 0 and row0 + rows < c.h and row0 < y0 and y1 < row0 + rows and f0 < y0, c.id


def test_the_old_flows_hold_every_special_value(oracle):
    for acc in K.ACC_COMPAT:
        for (w, h, rows, _) in acc.items:
            old, want = K.acc_compat_want(oracle, w, h, acc.win)
            kinds = {k for k, v in K.flow_kinds(old).items() if v}
            assert "nan" in kinds, (acc.id, w, h)
            if w * h >= 35:
                assert kinds == ALL_KINDS, (acc.id, w, h, kinds)
                # the launch's result keeps them apart: NaN, Inf and 1e30 swallow the addend, -0.0 takes it
                assert np.isnan(want).any() and np.isinf(want).any() and (np.abs(want) >= np.float32(9e29)).any()
    for (w, h, win) in K.ITER_SHAPES:
        kinds = {k for k, v in K.flow_kinds(K.iter_inputs(oracle, w, h, win)["old"]).items() if v}
        assert kinds == ALL_KINDS if w * h >= 35 else "nan" in kinds, (w, h, win, kinds)
    for c in (K.ROWS_MISS,):
        assert {k for k, v in K.flow_kinds(K.rows_inputs(oracle, c)["old"]).items() if v} == ALL_KINDS


def test_a_warp_case_meets_every_branch_of_the_warp(oracle):
    best = None
    for (w, h, win, rows, _, _) in K.WARP:
        _, flow = K.warp_flow(oracle, w, h, win)
        cen = ih.warp_census(flow, w, h, K.ITER_SCALE)
        if all(cen[k] > 0 for k in ih.CENSUS_KEYS):
            best = (w, h, cen)
    assert best is not None, "no warp case has every key of the census above 0"
    # ... and so does the flow an accumulating launch with d_warp_out leaves
    d = K.iter_inputs(oracle, K.edge_w(9), 67, 9)
    cen = ih.warp_census(K.add_ref(d["old"], d["delta"]), K.edge_w(9), 67, K.ITER_SCALE)
    assert all(cen[k] > 0 for k in ih.CENSUS_KEYS), cen


def test_the_guard_zeroes_some_pixels_and_not_all(oracle):
    w, h, win = K.GUARD_CASE
    p, n = K.frames(w, h)
    mask = ih.guarded_mask(oracle, p, win, ih.MIN_DET)
    assert 0 < int(mask.sum()) < mask.size, int(mask.sum())
    guarded, plain = K.level_ref(oracle, p, n, win, "lk_float", ih.MIN_DET), K.level_ref(oracle, p, n, win, "lk_float")
    assert (guarded[mask] == 0).all() and np.array_equal(guarded[~mask].view(np.uint32), plain[~mask].view(np.uint32))
    assert not np.array_equal(guarded.view(np.uint32), plain.view(np.uint32)), "the guard changes nothing: the case cannot tell the two values apart"
    for c in K.PLAIN:
        if c.min_det:
            m = ih.guarded_mask(oracle, K.frames(c.w, c.h, c.kind)[0], c.win, c.min_det)
            assert 0 < int(m.sum()) < m.size, (c.id, int(m.sum()))


def test_the_row_window_cases_are_with_and_without_a_missing_row(oracle):
    for c, missing in ((K.ROWS_NO_MISS, False), (K.ROWS_MISS, True)):
        d = K.rows_inputs(oracle, c)
        row0, rows, y0, y1, f0 = c["rows"]
        assert 0 < row0 and row0 + rows < c["h"] and row0 + (c["win"] >> 1) + 1 <= y0 and y1 + (c["win"] >> 1) + 1 <= row0 + rows and f0 < y0
        needs = d["needs"][y0:y1]
        if missing:
            assert needs.any(), "no pixel of the out rows needs a row outside the window"
            assert 2 * int((~needs).sum()) >= needs.size, f"{int((~needs).sum())} of {needs.size} out pixels are compared: less than half"
        else:
            assert not needs.any(), f"{int(needs.sum())} pixels need a row outside the window"
        assert not (c["preload"] >> c["bit"]) & 1


def test_warp_rows_is_the_oracles_warp_on_whole_levels(oracle):
    for (w, h, win, _, _, _) in K.WARP:
        src, flow = K.warp_flow(oracle, w, h, win)
        for scale in (K.ITER_SCALE, np.float32(-0.75)):
            got, needs = K.warp_rows(src, flow, scale)
            assert not needs.any()
            assert np.array_equal(got, oracle.warp_bilinear_u8(src, flow, scale)), (w, h, float(scale))
    # on a window, pixels that need no outside row are the whole level's
    c = K.ROWS_MISS
    d = K.rows_inputs(oracle, c)
    row0, rows = c["rows"][:2]
    got, needs = K.warp_rows(d["next"], d["flow"], K.ITER_SCALE, row0, row0 + rows)
    assert np.array_equal(got[~needs], d["warped"][~needs]) and (got[needs] != d["warped"][needs]).any()


def test_shift_ref_forms_the_vector_exactly(oracle):
    img = K.frames(37, 21)[1]
    assert np.array_equal(K.shift_ref(oracle, img, (0.0, 0.0)), img)
    assert np.array_equal(K.shift_ref(oracle, img, None), img)
    moved = K.shift_ref(oracle, img, (-2.5, 1.25))       # target ((int)(x - 2.5), (int)(y + 1.25)), truncated toward zero
    assert np.array_equal(moved[3:19, 5:30], img[4:20, 2:27])          # (int)(5 - 2.5) = 2, (int)(3 + 1.25) = 4
    out = K.shift_ref(oracle, img, K.uv_of("out", 37))   # every target outside: own byte while 3 (y w + x) < w h, else 0
    pos = np.arange(37 * 21).reshape(21, 37)
    assert np.array_equal(out, np.where(3 * pos < 37 * 21, img, 0))
    assert np.array_equal(K.shift_ref(oracle, img, K.uv_of("nan", 37)), out)
