"""CPU, referee only: tests/temporal_ref.py against the consequences that "temporal noise filter" of include/ofx.h states, its
rounding and its special values; the inputs of tests/temporal_cases.py reach every branch; and what the filter is for -- the noise
experiment with true fields, with zero fields and with none of the patch test."""
import numpy as np
import pytest

import temporal_cases as K
import temporal_ref as T

UNIFORM = np.full(256, 256, np.uint16)


def shifted(img, dx, dy):
    """img seen dx, dy pixels away, the border replicated"""
    h, w = img.shape[:2]
    return img[np.clip(np.arange(h) + dy, 0, h - 1)][:, np.clip(np.arange(w) + dx, 0, w - 1)]


@pytest.mark.parametrize("channels", [1, 3])
def test_zero_weights_copy_the_centre_and_zero_fields_on_the_centre_give_the_centre(channels):
    for w, h in K.SIZES:
        _, c, planes, fields, _, _ = K.case(w, h, channels, 3, "random", "all 0", 17)
        out, stats = T.temporal_filter(c, planes, fields, np.zeros(256, np.uint16), 17)
        assert np.array_equal(out, c) and stats[5] == w * h and stats[6] == 0 and stats[7] == 0 and stats[0] == w * h
        zero = [np.zeros((h, w, 2), np.float32)] * 2
        for table in K.tables().values():
            out, stats = T.temporal_filter(c, [c, c], zero, table, 3)
            assert np.array_equal(out, c) and stats[6] == 0 and stats[1] == stats[2] == 0
            assert stats[7] == 2 * w * h * int(table[0])          # every patch difference is 0


@pytest.mark.parametrize("channels", [1, 3])
def test_a_whole_pixel_field_fetches_a_shifted_copy(channels):
    w, h = 23, 11
    c, n = K.image(w, h, channels, 1), K.image(w, h, channels, 2)
    for dx, dy in ((2, -1), (-3, 2), (0, 1)):
        f = np.zeros((h, w, 2), np.float32)
        f[..., 0], f[..., 1] = dx, dy
        m, N0, usable, _ = T.patch_test(c, n, f)
        want = shifted(n.reshape(h, w, channels), dx, dy)
        assert np.array_equal(N0[usable], want[usable])
        y, x = np.mgrid[0:h, 0:w]
        assert np.array_equal(usable, (x + dx >= 0) & (x + dx < w) & (y + dy >= 0) & (y + dy < h))
        # wc = 1 against a weight of 256 everywhere: the rounded mean of (c + 256 n) / 257
        out, _ = T.temporal_filter(c, [n], [f], UNIFORM, 1)
        mean = (2 * (c.astype(np.int64) + 256 * want.reshape(c.shape).astype(np.int64)) + 257) // (2 * 257)
        assert np.array_equal(out[usable], mean[usable]) and np.array_equal(out[~usable], c[~usable])


def test_appending_a_neighbour_without_weight_changes_only_its_own_count():
    for channels in (1, 3):
        name, c, planes, fields, table, wc = K.case(67, 9, channels, 2, "ramp", "sigma 10", 256)
        c, planes = c // 3, [p // 3 for p in planes]                   # (at most 85)
        out, stats = T.temporal_filter(c, planes, fields, table, wc)
        # a neighbour so different that its patch difference has weight 0 everywhere under this table, usable or not
        far = np.full_like(c, 255)
        extra = K.field("special", 67, 9, 3)
        assert T.weights_for(10.0)[100:].max() == 0 and T.patch_test(c, far, extra)[0].min() >= 100
        out3, stats3 = T.temporal_filter(c, planes + [far], fields + [extra], table, wc)
        assert np.array_equal(out3, out)
        assert stats3[3] == int((~T.positions(extra, 67, 9)[3]).sum()) > 0
        stats3[3] = 0
        assert stats3.tolist() == stats.tolist()


def test_ties_round_to_even():
    w, h = 40, 3
    f = np.zeros((h, w, 2), np.float32)
    k = np.arange(w) - 20
    f[..., 0] = ((k + 0.5) / 32.0).astype(np.float32)[None, :]          # exact in float32
    f[..., 1] = ((k[::-1] + 0.5) / 32.0).astype(np.float32)[None, :]
    qx, qy, defined, _ = T.positions(f, w, h)
    want = np.where(k % 2 == 0, k, k + 1)                                # k + 0.5 -> the even neighbour
    assert defined.all() and np.array_equal(qx[0] - 32 * np.arange(w), want) and np.array_equal(qy[1] - 32, want[::-1])


def test_the_special_values_of_the_geometry():
    w, h = len(K.SPECIAL), 2
    f = np.zeros((h, w, 2), np.float32)
    f[0, :, 0], f[1, :, 1] = K.SPECIAL, K.SPECIAL
    with np.errstate(all="ignore"):
        qx, qy, defined, usable = T.positions(f, w, h)
    want_defined = np.array([1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], bool)     # -0, the denormals and +-2^20 are; the rest is not
    assert np.array_equal(defined[0], want_defined) and np.array_equal(defined[1], want_defined)
    x = 32 * np.arange(w)
    assert np.array_equal(qx[0, :3], x[:3]) and np.array_equal(qy[1, :3], [32, 32, 32])      # -0 and the denormals round to 0
    assert qx[0, 3] == x[3] + (1 << 25) and qx[0, 4] == x[4] - (1 << 25) and qy[1, 3] == 32 + (1 << 25)
    assert np.array_equal(usable[0], [1, 1, 1] + [0] * 9) and np.array_equal(usable[1], [1, 1, 1] + [0] * 9)
    assert (qx[~defined] == 0).all() and (qy[~defined] == 0).all()
    # and with denormals flushed before the product, the positions are the same
    g = np.where(np.abs(f) < np.finfo(np.float32).tiny, np.float32(0.0), f)
    with np.errstate(all="ignore"):
        assert all(np.array_equal(a, b) for a, b in zip(T.positions(g, w, h), (qx, qy, defined, usable)))


def test_the_shared_cases_reach_every_branch():
    seen = set()
    for channels in (1, 3):
        for w, h in K.SIZES:
            for name, c, planes, fields, table, wc in K.ladder(w, h, channels):
                den = np.full((h, w), wc, np.int64)
                for k, (p, f) in enumerate(zip(planes, fields)):
                    with np.errstate(all="ignore"):
                        qx, qy, defined, usable = T.positions(f, w, h)
                        m, N0, _, interior = T.patch_test(c, p, f)
                    den += np.where(usable, table[m].astype(np.int64), 0)
                    seen |= {("undefined", bool((~defined).any())), ("out of range", bool((defined & ~usable).any())),
                             ("interior taps", bool((usable & interior).any())), ("border taps", bool((usable & ~interior).any())),
                             ("fraction", bool((usable & ((qx & 31) != 0) & ((qy & 31) != 0)).any())),
                             ("at 0", bool((usable & (qx == 0)).any() and (usable & (qy == 0)).any())),
                             ("at the end", bool((usable & (qx == 32 * (w - 1))).any() and (usable & (qy == 32 * (h - 1))).any())),
                             ("m saturates", bool((m == 255).any())), ("m = 0", bool((m == 0).any())),
                             ("m in the table's slope", bool(((m > 15) & (m < 40)).any()))}
                    if w >= 64:
                        # the two tap paths meet inside one wave: 64 consecutive quads, numbered row by row
                        qpr = (w + 3) // 4
                        wave = (np.arange(h)[:, None] * qpr + np.arange(w)[None, :] // 4) // 64
                        for g in np.unique(wave):
                            u = usable & (wave == g)
                            seen.add(("both paths in a wave", bool((u & interior).any() and (u & ~interior).any())))
                seen |= {("no weight", bool((den == wc).any())), ("full weight", bool((den == wc + 256 * len(planes)).any())),
                         ("tail quad", w % 4 != 0), ("blocks", (w + 3) // 4 * h > 256), ("S", len(planes)), ("wc", wc)}
    for what in ("undefined", "out of range", "interior taps", "border taps", "fraction", "at 0", "at the end", "m saturates", "m = 0",
                 "m in the table's slope", "both paths in a wave", "no weight", "full weight", "tail quad", "blocks"):
        assert (what, True) in seen, what
    assert {("S", s) for s in (1, 2, 3, 4)} <= seen and {("wc", v) for v in (1, 37, 256)} <= seen


def test_the_division_case_holds_every_pair_of_values():
    name, a, planes, fields, table, wc = K.division_case(37)
    assert a.shape == (768, 768) and len(set(zip(a[1::3, 1::3].reshape(-1).tolist(), planes[0][1::3, 1::3].reshape(-1).tolist()))) == 65536
    m, N0, usable, _ = T.patch_test(a, planes[0], fields[0])
    # at the middle of each 3 x 3 cell both patches are flat: m = |a - b|, so every difference meets its table entry
    assert usable.all() and np.array_equal(m[1::3, 1::3], np.abs(a[1::3, 1::3].astype(np.int64) - planes[0][1::3, 1::3]))
    out, _ = T.temporal_filter(a, planes, fields, table, wc)
    A, B = a[1::3, 1::3].astype(np.int64), planes[0][1::3, 1::3].astype(np.int64)
    wk = table[np.abs(A - B)].astype(np.int64)
    assert np.array_equal(out[1::3, 1::3], np.floor((wc * A + wk * B) / (wc + wk) + 0.5).astype(np.uint8))    # exact: den <= 293


# ---- what the filter is for ------------------------------------------------------------------------------------------------------

def mse(a, b, border=8):
    d = np.asarray(a, np.float64)[border:-border, border:-border] - np.asarray(b, np.float64)[border:-border, border:-border]
    return float((d * d).mean())


def true_fields(w, h, step=(3, 2)):
    """frame f shows the texture at x + f step: frame f-1 shows the same point at x + step, frame f+1 at x - step"""
    prev, nxt = np.zeros((h, w, 2), np.float32), np.zeros((h, w, 2), np.float32)
    prev[..., 0], prev[..., 1] = step
    nxt[..., 0], nxt[..., 1] = -step[0], -step[1]
    return [prev, nxt]


@pytest.mark.parametrize("sigma", [5, 10, 20])
def test_the_noise_experiment(sigma):
    """128 x 96, three frames panning by (3, 2), Gaussian noise: error against the clean middle frame over the noisy frame's.
    True whole-pixel fields: three equal samples allow 1/3; asserted <= 0.40 at sigma 10 (rounding and the clip at 0 / 255).
    Zero fields on the sharp texture: the patch test keeps the filter from hurting, <= 1.05; a uniform table does hurt."""
    noisy, clean = K.pan_clip(3, 128, 96, 1, sigma)
    assert clean.min() >= 40 and clean.max() <= 215
    base = mse(noisy[1], clean[1])
    table = T.weights_for(sigma)
    zero = [np.zeros((96, 128, 2), np.float32)] * 2
    near = [noisy[0], noisy[2]]
    true = mse(T.temporal_filter(noisy[1], near, true_fields(128, 96), table)[0], clean[1]) / base
    still = mse(T.temporal_filter(noisy[1], near, zero, table)[0], clean[1]) / base
    blind = mse(T.temporal_filter(noisy[1], near, zero, UNIFORM)[0], clean[1]) / base
    print(f"sigma {sigma}: true fields {true:.3f}, zero fields {still:.3f}, zero fields without the patch test {blind:.3f}")
    if sigma == 10:
        assert true <= 0.40
    assert still <= 1.05
    assert blind > still


def clip_mse(a, b, border=8):
    d = np.asarray(a, np.float64)[:, border:-border, border:-border] - np.asarray(b, np.float64)[:, border:-border, border:-border]
    return float((d * d).mean())


def test_the_noise_experiment_with_fields_estimated_from_the_noisy_frames(oracle):
    """What tests/test_gpu_temporal.py measures on the device, on the CPU: the 5-frame 192 x 128 pan at sigma 10, every pair's
    displacement from the NOISY frames by the coarse-to-fine dense flow with the 5 x 5 flow median (median_ref over dense_ref: 4 levels,
    window 9, 3 iterations, min_det 1), forwards and in reverse frame order, then temporal_ref.denoise_rings.  The error against the
    clean frames must be below the noisy frames' and below that of the same filter with zero fields."""
    import median_ref as M

    n, w, h, sigma = 5, 192, 128, 10
    noisy, clean = K.pan_clip(n, w, h, 1, sigma)
    flow = lambda a, b: M.dense_displacement_median(oracle, a, b, 4, 9, 3, 1.0, None, 2)
    fwd = np.stack([flow(noisy[p], noisy[p + 1]) for p in range(n - 1)])
    back = noisy[::-1]
    bwd = np.stack([flow(back[p], back[p + 1]) for p in range(n - 1)])            # the reversed run: bwd[N-2-p] is frame p+1 -> p
    assert fwd.shape == bwd.shape == (n - 1, h, w, 2)
    table = T.weights_for(sigma)
    out = np.stack([o for o, _ in T.denoise_rings(noisy, fwd, bwd, table)])
    zero = np.zeros_like(fwd)
    still = np.stack([o for o, _ in T.denoise_rings(noisy, zero, zero, table)])
    base = clip_mse(noisy, clean)
    r_flow, r_zero = clip_mse(out, clean) / base, clip_mse(still, clean) / base
    print(f"sigma {sigma}: error over the noisy frames' error: dense flow with the 5x5 median on the noisy frames {r_flow:.3f}, zero fields {r_zero:.3f}")
    assert r_flow < 1.0
    assert r_flow < r_zero
