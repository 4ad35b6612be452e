"""The inputs of the temporal-filter tests, shared by tests/test_temporal_ref.py (CPU: the referee reaches every branch on them) and
tests/test_gpu_temporal.py (the device against the referee).  A case is (name, centre, planes, fields, weights, centre_weight)."""
import numpy as np

import temporal_ref as T

# below a patch (every tap clamped) | a tail quad, odd width, rows starting at every address mod 4 | 297 quads: more than one block
SIZES = [(1, 1), (3, 2), (4, 1), (5, 3), (67, 9), (131, 9)]
KINDS = ["zero", "whole", "random", "ramp", "special", "edge"]
TWO20 = np.float32(1048576.0)
SPECIAL = np.array([-0.0, 1e-45, -1e-40, TWO20, -TWO20, np.nextafter(TWO20, np.float32(np.inf)), -np.nextafter(TWO20, np.float32(np.inf)),
                    np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32)


def image(w, h, channels, seed):
    """a smooth texture plus noise, so that patch differences spread over the table and not only saturate"""
    rng = np.random.RandomState(1000 + seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 128 + 60 * np.sin(0.21 * x + 0.1 * seed) * np.cos(0.17 * y) + 30 * np.sin(0.05 * (x + 2 * y))
    img = base[:, :, None] + 10.0 * np.arange(channels)[None, None, :] + rng.normal(0.0, 6.0, (h, w, channels))
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return img if channels == 3 else img[:, :, 0]


def field(kind, w, h, seed):
    rng = np.random.RandomState(2000 + seed)
    y, x = np.mgrid[0:h, 0:w]
    f = np.zeros((h, w, 2), np.float32)
    if kind == "whole":
        f[..., 0], f[..., 1] = (2, -1) if seed % 2 else (-1, 1)
    elif kind == "random":
        f[...] = rng.uniform(-3.0, 3.0, (h, w, 2)).astype(np.float32)
    elif kind == "ramp":
        # the border pixels leave the frame on each side, their neighbours land on the border, the middle stays interior
        f[..., 0] = (2.0 * x / max(w - 1, 1) - 1.0) * 2.3
        f[..., 1] = (2.0 * y / max(h - 1, 1) - 1.0) * 1.7
    elif kind == "special":
        f[...] = rng.uniform(-3.0, 3.0, (h, w, 2)).astype(np.float32)
        n = max(2, (w * h) // 3)
        at = rng.randint(0, w * h * 2, n)
        f.reshape(-1)[at] = SPECIAL[np.arange(n) % len(SPECIAL)]
    elif kind == "edge":
        # positions exactly at 0 and at 32 (size - 1)
        f[..., 0] = np.where(y % 2 == 0, -x, (w - 1) - x)
        f[..., 1] = np.where(x % 2 == 0, -y, (h - 1) - y)
    else:
        assert kind == "zero"
    return f


def tables():
    rng = np.random.RandomState(7)
    return {"all 256": np.full(256, 256, np.uint16), "all 0": np.zeros(256, np.uint16), "sigma 10": T.weights_for(10.0),
            "random": rng.randint(0, 257, 256).astype(np.uint16)}


def case(w, h, channels, S, kind, table, wc, seed=0, same=False, own=False):
    """S neighbours with fields of `kind` (neighbour k's seed differs); same: neighbours 0 and 1 are one plane; own: neighbour 0 is
    the centre itself"""
    centre = image(w, h, channels, seed)
    planes = [image(w, h, channels, seed + 1 + k) for k in range(S)]
    if own:
        planes[0] = centre
    if same and S >= 2:
        planes[1] = planes[0]
    fields = [field(kind, w, h, seed + 10 * k) for k in range(S)]
    name = f"{w}x{h} C={channels} S={S} {kind} {table} wc={wc}" + (" same" if same else "") + (" own" if own else "")
    return name, centre, planes, fields, tables()[table], wc


def ladder(w, h, channels):
    """what test_gpu_temporal runs at one size and channel count: every kind of field, S = 1 .. 4, every table, wc 1 and 256"""
    names = list(tables())
    out = []
    for i, kind in enumerate(KINDS):
        S = 1 + i % 4
        out.append(case(w, h, channels, S, kind, names[i % 4], 256 if i % 2 else 1, seed=i))
        out.append(case(w, h, channels, 1 + (i + 2) % 4, kind, names[(i + 1) % 4], 1 if i % 2 else 256, seed=20 + i, same=i % 2 == 0, own=i % 3 == 0))
    out.append(case(w, h, channels, 4, "random", "sigma 10", 256, seed=40))
    out.append(case(w, h, channels, 2, "ramp", "random", 37, seed=41, same=True))
    out.append(case(w, h, channels, 3, "special", "all 256", 256, seed=42))
    out.append(case(w, h, channels, 2, "zero", "sigma 10", 256, seed=43, own=True))
    # black against white: the mean patch difference reaches 255 and is clipped there
    name, centre, planes, fields, table, wc = case(w, h, channels, 2, "random", "random", 256, seed=44)
    centre = np.where(np.arange(w)[None, :] < (w + 1) // 2, 0, 255).astype(np.uint8)[:, :, None].repeat(h, 0).repeat(channels, 2).reshape(centre.shape)
    out.append((name + " black and white", centre, [255 - centre, planes[1]], [np.zeros_like(fields[0]), fields[1]], table, wc))
    return out


def division_case(wc, seed=5):
    """every pair (a, b) of centre and neighbour values: a = x, b = y on a 256 x 256 grid enlarged 3 x 3, zero field, random table"""
    a = np.repeat(np.repeat(np.arange(256, dtype=np.uint8)[None, :].repeat(256, 0), 3, 0), 3, 1)
    b = np.repeat(np.repeat(np.arange(256, dtype=np.uint8)[:, None].repeat(256, 1), 3, 0), 3, 1)
    table = np.random.RandomState(seed).randint(0, 257, 256).astype(np.uint16)
    return f"division wc={wc}", a, [b], [np.zeros((768, 768, 2), np.float32)], table, wc


def pan_clip(n, w, h, channels, sigma, seed=0, step=(3, 2)):
    """(noisy uint8 [n, h, w(, 3)], clean float64 alike): a band-limited texture with values within 48 .. 208 panning by `step` px a
    frame -- frame f shows the texture at (x + f step) -- plus Gaussian noise, rounded and clipped"""
    rng = np.random.RandomState(300 + seed)
    big_h, big_w = h + n * abs(step[1]) + 8, w + n * abs(step[0]) + 8
    tex = np.zeros((big_h, big_w, channels))
    y, x = np.mgrid[0:big_h, 0:big_w].astype(np.float64)
    for c in range(channels):
        acc = np.zeros((big_h, big_w))
        for _ in range(12):
            fx, fy = rng.uniform(-0.9, 0.9, 2)       # radians per pixel: well below Nyquist
            acc += rng.uniform(0.5, 1.0) * np.sin(fx * x + fy * y + rng.uniform(0, 2 * np.pi))
        tex[:, :, c] = 128.0 + 80.0 * acc / np.abs(acc).max()
    clean = np.stack([tex[f * step[1]:f * step[1] + h, f * step[0]:f * step[0] + w] for f in range(n)])
    noisy = np.clip(np.rint(clean + rng.normal(0.0, sigma, clean.shape)), 0, 255).astype(np.uint8)
    if channels == 1:
        clean, noisy = clean[..., 0], noisy[..., 0]
    return noisy, clean
