"""CPU: the referee of the displacement chain (tests/chain_ref.py) against the referee of the forward-backward check, whose tap
geometry and blend are pinned against the oracle; the consequences the definition states; the inputs of tests/chain_cases.py reach
the branches they are named for; and what a reach of two frames buys the temporal filter, on the referees alone."""
import numpy as np
import pytest

import chain_cases as K
import chain_ref as R
import consistency_ref
import temporal_cases

F32 = np.float32
BIG = [s for s in K.SIZES if s[0] * s[1] > 100]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(got, want, what):
    got, want = bits(got) if np.asarray(got).dtype == F32 else np.asarray(got), bits(want) if np.asarray(want).dtype == F32 else np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)}/{got.size} differ, first at {bad[:3].tolist()}"


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_two_links_against_the_consistency_referee(size, kind):
    """r_u and the classes: consistency's classes 2 and 3 before its step 6 are the chain's steps 2 and 3; its step 7 is not the
    chain's step 5, so pixels it decides there are compared through r_u alone"""
    w, h = size
    d0, d1 = K.links(kind, w, h, 2)
    dst, mask, stats, (p,) = R.chain([d0, d1], parts=True)
    cmask, _, _, cp = consistency_ref.consistency(d0, d1, 1.0, 0.0, 0.0, parts=True)
    same(p["px"], cp["px"], "px")
    same(p["py"], cp["py"], "py")
    same(p["ru"], cp["ru"], "r_u")
    early = ~p["live"]                                       # decided before the second link is read: consistency's steps 2 and 3
    assert np.isin(cmask[early], (consistency_ref.LEAVES, consistency_ref.UNDEFINED)).all() and np.array_equal(mask[early], cmask[early])
    assert (mask[p["live"] & ~p["overflow"]] == R.OK).all() and (mask[p["overflow"]] == R.UNDEFINED).all()
    assert stats.tolist() == [w * h, int((mask == 2).sum()), int((mask == 3).sum()), int((mask == 0).sum())] and stats[1:].sum() == w * h


@pytest.mark.parametrize("L", [2, 3, 4])
def test_whole_pixel_constant_fields_add_exactly_in_the_interior(L):
    w, h = 67, 33
    rng = np.random.default_rng(L)
    t = rng.integers(-3, 4, (L, 2))
    links = [np.broadcast_to(t[j].astype(F32), (h, w, 2)) for j in range(L)]
    dst, mask, stats = R.chain(links)
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    inside = np.ones((h, w), bool)
    for j in range(1, L):                                    # the path stays inside: the position after j links lies in the frame
        px, py = xs + t[:j, 0].sum(), ys + t[:j, 1].sum()
        inside &= (px >= 0) & (px <= w - 1) & (py >= 0) & (py <= h - 1)
    assert inside.any() and not inside.all()
    assert np.array_equal(mask == R.OK, inside) and (mask[~inside] == R.LEAVES).all()
    same(dst[inside], np.broadcast_to(t.sum(0).astype(F32), (int(inside.sum()), 2)), "the sum")


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("L", [3, 4])
def test_a_chain_is_the_left_fold_of_two_link_chains(L, kind):
    for w, h in K.SIZES:
        links = K.links(kind, w, h, L)
        dst, mask, stats = R.chain(links)
        acc = links[0]
        for j in range(1, L):
            acc, m2, _ = R.chain([acc, links[j]])
        same(acc, dst, f"{kind} {w}x{h} L={L}")
        assert np.array_equal(m2 == R.OK, mask == R.OK)     # (a fold's last call cannot tell why an earlier one gave a vector up)


@pytest.mark.parametrize("kind", K.KINDS)
def test_dead_vectors_have_the_one_bit_pattern_and_ok_vectors_are_finite(kind):
    for w, h in K.SIZES:
        for L in (2, 3, 4):
            dst, mask, _ = R.chain(K.links(kind, w, h, L))
            b = bits(dst)
            assert (b[mask != R.OK] == R.DEAD_BITS).all()
            assert np.isfinite(dst[mask == R.OK]).all()
            assert set(np.unique(mask).tolist()) <= {R.OK, R.LEAVES, R.UNDEFINED}


@pytest.mark.parametrize("size", BIG, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_kind_reaches_the_branch_it_is_named_for(size):
    w, h = size
    for L in (2, 3, 4):
        run = {kind: R.chain(K.links(kind, w, h, L), parts=True) for kind in K.KINDS}
        dst, mask, stats, parts = run["integers"]
        assert stats[3] > 0 and stats[1] > 0
        fr = [np.modf(p["px"][p["live"]])[0] for p in parts]
        assert all((f == 0).all() for f in fr), "integers: every fraction is 0"
        dst, mask, stats, parts = run["inverse"]
        assert stats[3] > w * h // 2 and any((np.modf(p["px"][p["live"]])[0] != 0).any() for p in parts)
        dst, mask, stats, parts = run["borders"]
        assert stats[1] > w * h // 8 and stats[3] > 0
        gone = parts[0]["left"]                              # over every border at the first step, and some at every later one
        assert (parts[0]["px"][gone] < 0).any() and (parts[0]["px"][gone] > w - 1).any() and (parts[0]["py"][gone] < 0).any() and (parts[0]["py"][gone] > h - 1).any()
        assert all(p["left"].any() for p in parts)
        dst, mask, stats, parts = run["nonfinite"]
        assert stats[2] > 0 and stats[3] > 0
        assert parts[0]["undefined"].any() and any(p["overflow"].any() for p in parts), "a bad vector so far, and a bad tap"
        assert (bits(np.stack(K.links("nonfinite", w, h, L))) == R.DEAD_BITS).any(), "the dead pattern is among the inputs"
        dst, mask, stats, parts = run["edge"]
        p = parts[0]
        assert (p["live"] & (p["x0"] == w - 1)).any() and (p["live"] & (p["y0"] == h - 1)).any(), "taps in the last column and row"
        last_col = p["live"] & (p["x0"] == w - 1)
        assert np.isfinite(dst[last_col & (mask == R.OK)]).all() and (last_col & (mask == R.OK)).any(), "the NaN behind the last column stays out"
        assert np.isnan(K.links("edge", w, h, L)[1][:, 0]).all()
        dst, mask, stats, parts = run["overflow"]
        assert parts[-1]["overflow"].any() and stats[2] > 0 and np.isfinite(np.stack(K.links("overflow", w, h, L))).all()
        dst, mask, stats, parts = run["denormal"]
        tiny = np.finfo(F32).tiny
        ok = dst[mask == R.OK]
        assert ((np.abs(ok) < tiny) & (ok != 0)).any(), "denormal results"
        assert ((np.abs(parts[0]["ru"]) < tiny) & (parts[0]["ru"] != 0)).any()


def test_the_ring_is_the_chain_of_every_window():
    ring = np.stack([K.links("inverse", 67, 33, 4, seed=s)[0] for s in range(5)])
    for span in (2, 3, 4):
        out = R.chain_ring(ring, span)
        assert out.shape == (5 - span + 1, 33, 67, 2)
        for p in range(len(out)):
            same(out[p], R.chain(list(ring[p:p + span]))[0], f"span {span}, entry {p}")


def test_reach_two_beats_reach_one_on_the_referees():
    """pan_clip(7, 192, 128, 1, 10) with the true fields: the error over the noisy frames' error, frames 2 to 4, border 16.  It
    measured 0.198 (reach 2) against 0.330 (reach 1)."""
    import temporal_ref as T

    n, w, h, sigma = 7, 192, 128, 10
    noisy, clean = temporal_cases.pan_clip(n, w, h, 1, sigma)
    fwd = np.broadcast_to(np.array([3, 2], F32), (n - 1, h, w, 2))       # frame f shows the texture at x + 3 f: f + 1 shows x's point at x - 3 ...
    fwd, bwd = -fwd, fwd.copy()                                          # ... so the displacement f -> f + 1 is (-3, -2)
    table = T.weights_for(sigma)

    def ratio(res):
        out = np.stack([r[0] for r in res]).astype(np.float64)
        sl = (slice(2, 5), slice(16, -16), slice(16, -16))
        return float(((out[sl] - clean[sl]) ** 2).mean() / ((noisy[sl].astype(np.float64) - clean[sl]) ** 2).mean())

    r1, r2 = ratio(R.denoise_rings(noisy, fwd, bwd, table, 1)), ratio(R.denoise_rings(noisy, fwd, bwd, table, 2))
    print(f"error over the noisy frames' error: reach 1 {r1:.3f}, reach 2 {r2:.3f}")
    assert r2 < r1 < 1.0
