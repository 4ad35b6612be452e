"""The seeded inputs the CPU and the GPU tests of the displacement chain share (tests/test_chain_ref.py shows that every kind reaches
the branch it is named for).  Not a test module and not a conftest: tests import it."""
import functools

import numpy as np

F32 = np.float32
SIZES = [(1, 1), (4, 1), (1, 5), (5, 3), (67, 33), (130, 9), (257, 40)]   # (w, h); the last takes three blocks and has a ragged row end
KINDS = ["integers", "inverse", "borders", "nonfinite", "edge", "overflow", "denormal"]
DEAD = np.array([0x7FC00000], np.uint32).view(F32)[0]
NONFINITE = np.array([np.nan, np.inf, -np.inf, 1e12, -1e12, 1e30, -1e30, DEAD], F32)


@functools.lru_cache(maxsize=None)
def links(kind, w, h, L, seed=0):
    """a tuple of L read-only float32 fields [h, w, 2], in pixels"""
    rng = np.random.default_rng(1000 * seed + 131 * w + 17 * h + 7 * KINDS.index(kind) + L)
    xs, ys = np.arange(w)[None, :], np.arange(h)[:, None]
    if kind == "integers":                                   # whole pixels, constant and random in turn: every fraction is 0
        out = [np.broadcast_to(rng.integers(-2, 3, 2), (h, w, 2)).astype(F32) if j % 2 == 0 else rng.integers(-3, 4, (h, w, 2)).astype(F32)
               for j in range(L)]
    elif kind == "edge":                                     # vectors that land exactly on the last column or row; NaN behind it
        out = []
        for j in range(L):
            f = rng.choice([-0.5, 0.0, 0.5], (h, w, 2)).astype(F32)
            if j == 0:
                pick = rng.integers(0, 3, (h, w))
                f[..., 0] = np.where(pick == 0, (w - 1 - xs).astype(F32), f[..., 0])
                f[..., 1] = np.where(pick == 1, (h - 1 - ys).astype(F32), f[..., 1])
            elif j == 1:
                f[..., 0] = np.where(xs == w - 1, F32(0.0), f[..., 0])     # stay in the last column for the next link
                if w > 1:
                    f[:, 0, :] = np.nan                      # the memory neighbour of column w - 1 of the row above
            out.append(f)
    elif kind == "denormal":                                 # denormal vectors, and fractions that make denormal products
        out = [((rng.integers(-3, 4, (h, w, 2)) * 1e-42).astype(F32) + np.where(rng.random((h, w, 2)) < 0.3, F32(1e-39), F32(0))).astype(F32)
               for _ in range(L)]
        out[0][rng.random((h, w)) < 0.3] += F32(0.25)        # a fraction: fx * (b01 - b00) is a denormal product
    else:
        t = rng.uniform(-2.5, 2.5, 2)
        out = [((t if j % 2 == 0 else -t) + rng.normal(0.0, 0.35, (h, w, 2))).astype(F32) for j in range(L)]   # "inverse"
        if kind == "borders":                                # one vector in three pushed beyond one of the four borders
            far = max(w, h) + 7.3
            for f in out:
                pick = rng.integers(0, 3, (h, w)) == 0
                side = rng.integers(0, 4, (h, w))
                f[..., 0] = np.where(pick & (side == 0), -far - xs, np.where(pick & (side == 1), (w - 1 - xs) + far, f[..., 0]))
                f[..., 1] = np.where(pick & (side == 2), -far - ys, np.where(pick & (side == 3), (h - 1 - ys) + far, f[..., 1]))
        elif kind == "nonfinite":                            # in 4 % of the components of every link
            for f in out:
                hit = rng.random((h, w, 2)) < 0.04
                f[hit] = NONFINITE[rng.integers(0, len(NONFINITE), int(hit.sum()))]
        elif kind == "overflow":                             # finite +-3e38 in the last link: where two taps differ in sign their
            out[L - 1][...] = rng.choice([-3e38, 3e38], (h, w, 2))   # difference leaves float32, r is Inf or NaN and step 5 fails
    out = [np.ascontiguousarray(o, F32) for o in out]
    for o in out:
        o.setflags(write=False)
    return tuple(out)
