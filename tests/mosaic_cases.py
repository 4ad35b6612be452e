"""The inputs of the frame-mosaic tests, shared by tests/test_mosaic_ref.py (CPU: the referee reaches every rule on them) and
tests/test_gpu_mosaic.py (the device against the referee).  A case is (name, srcs, models, (w, h)): srcs uint8 images, models nine
floats each, in priority order."""
import math

import numpy as np

from test_gpu_warp_persp import SHAPES, image, models_for  # noqa: F401  ((w, h, sw, sh): (1, 1, 3, 2) .. (262, 74, 259, 80))

LADDER_S = [1, 2, 5, 9]
HARD = ["horizon inside", "W = 0 at pixels", "W < 0 everywhere", "tiny W", "far", "limits"]
WAVE_PX = 256                                   # a wave: 64 lanes of four adjacent pixels, quads numbered row by row


def ladder(w, h, S, channels):
    """S sources of different sizes; the output's columns fall into S + 1 vertical bands of w // (S + 1) columns (the last takes the
    rest and stays uncovered); source k covers band order[k] and a column either side of it, a quarter pixel off the lattice, every
    second source slightly tilted; `order` is shuffled, so the priority decides in the columns two sources share"""
    bw = max(w // (S + 1), 1)
    order = np.random.RandomState(100 + S).permutation(S)
    t = 0.5 / max(w, h)
    srcs, models = [], []
    for k in range(S):
        x_lo = int(order[k]) * bw
        srcs.append(image(bw + 3, h + 3 + k % 3, channels, 7 * k + S))
        tilt = t if k % 2 else 0.0
        models.append((1.0, tilt, 1.25 - x_lo, -tilt, 1.0, 1.25, 0.0, 0.0, 1.0))
    return f"ladder S={S}", srcs, models, (w, h)


SHAKE = [(2.25, -1.5, 0.0), (3.5, 2.0, 0.0), (-4.0, 3.5, 0.0), (1.75, -5.0, 0.003), (-2.5, -4.25, 0.0)]        # (tx, ty, angle)


def shake(w, h, channels):
    """five sources of the output's own size, shifted by a few pixels in different directions: source 0 resolves the interior"""
    srcs = [image(w, h, channels, 31 + k) for k in range(len(SHAKE))]
    models = [(math.cos(a), -math.sin(a), tx, math.sin(a), math.cos(a), ty, 0.0, 0.0, 1.0) for tx, ty, a in SHAKE]
    return "shake", srcs, models, (w, h)


def hard_pairs(w, h, sw, sh, channels):
    """source 0 through each hard model of test_gpu_warp_persp.models_for, set against a second source that covers the whole output
    ("full") or only its left half and a column ("half": to its right nothing covers the pixels that source 0 leaves)"""
    by = dict(models_for(w, h, sw, sh))
    cases = []
    for name in HARD:
        for part, w1 in (("full", w + 2), ("half", max(w // 2, 1) + 2)):
            srcs = [image(sw, sh, channels, 3), image(w1, h + 2, channels, 5)]
            cases.append((f"{name}, {part}", srcs, [by[name], (1.0, 0.0, 0.75, 0.0, 1.0, 0.5, 0.0, 0.0, 1.0)], (w, h)))
    return cases


def waves(which):
    """the values of a `which` plane [h, w] per wave of the kernel's march: a list of 1-D arrays, one per 64 consecutive quads"""
    h, w = which.shape
    qpr = (w + 3) // 4
    padded = np.full((h, 4 * qpr), -1, np.int64)
    padded[:, :w] = which
    quads = padded.reshape(h * qpr, 4)
    return [q[q >= 0] for q in (quads[g:g + 64].reshape(-1) for g in range(0, len(quads), 64))]
