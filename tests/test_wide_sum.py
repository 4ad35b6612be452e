"""CPU: csrc/wide_sum.h on the host (tests/wide_sum_check.cpp) against Python ints -- the 128-bit -> float64 conversion equals
float(int), which rounds to nearest even in one step, and the two-halves add with a carry equals addition modulo 2^128."""
import os
import random
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64, M128 = (1 << 64) - 1, (1 << 128) - 1


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = tmp_path_factory.mktemp("wide") / "wide_sum_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "cuda_optical_flow_2_amd", "csrc"),
                    os.path.join(ROOT, "tests", "wide_sum_check.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        out = r.stdout.split("\n")
        assert r.returncode == 0 and out[len(lines)] == f"ok {len(lines)}", (r.returncode, out[-3:])
        return out[:len(lines)]

    return run


def halves(v):
    v &= M128
    return v >> 64, v & M64


def bits(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]


def check_conversion(ask, values):
    got = ask(["c %x %x" % halves(v) for v in values])
    bad = [(v, g, bits(float(v))) for v, g in zip(values, got) if g != bits(float(v))]
    assert not bad, (len(bad), bad[:3])


def test_powers_of_two_and_their_neighbours(ask):
    values = [0, 1, -1, (1 << 53) - 1, 1 << 53, (1 << 53) + 1, -(1 << 127), (1 << 127) - 1]
    for k in range(52, 127):
        for d in (-1, 0, 1):
            values += [(1 << k) + d, -((1 << k) + d)]
    check_conversion(ask, values)


def test_exact_ties_at_bit_53_go_to_even(ask):
    values = []
    for k in range(54, 127):                 # the value has k + 1 bits; the half sits at bit k - 53
        half = 1 << (k - 53)
        for mant in ((1 << 52) | 0x5A5A5A5A5A5A4, (1 << 52) | 0x5A5A5A5A5A5A5, (1 << 53) - 1, 1 << 52):   # even, odd, all ones, least
            v = (mant << (k - 52)) | half
            values += [v, -v]
            assert float(v) == float((mant + (mant & 1)) << (k - 52))
    check_conversion(ask, values)


def test_a_sticky_bit_far_below_the_tie_breaks_it(ask):
    """a double rounding through 64 bits would drop the bit 60 places below the half and round the tie to even"""
    values = []
    for k in range(114, 127):
        half = 1 << (k - 53)
        for mant in ((1 << 52) | 0x123456789ABCC, (1 << 52) | 0x123456789ABCD):
            tie = (mant << (k - 52)) | half
            for v in (tie | (half >> 60), tie - (half >> 60)):
                values += [v, -v]
            assert float(tie | (half >> 60)) == float((mant + 1) << (k - 52)) and float(tie - (half >> 60)) == float(mant << (k - 52))
    check_conversion(ask, values)


def test_random_values(ask):
    rng = random.Random(20240)
    values = []
    for _ in range(10000):
        v = rng.getrandbits(rng.randint(1, 127))
        values.append(-v if rng.random() < 0.5 else v)
    check_conversion(ask, values)


def test_the_add_with_a_carry_is_addition_modulo_2_to_the_128(ask):
    rng = random.Random(7)
    pairs = [(0, 0), (M64, 1), (-1, 1), (-1, -1), (1 << 64, -1), (-(1 << 127), -(1 << 127)), ((1 << 127) - 1, 1), (M64, M64), (-(1 << 64), M64)]
    for _ in range(4000):
        a, b = (rng.choice((-1, 1)) * rng.getrandbits(rng.choice((20, 63, 64, 65, 100, 127))) for _ in range(2))
        pairs.append((a, b))
        lo = rng.getrandbits(64)
        pairs.append(((rng.getrandbits(40) << 64) | lo, -(rng.getrandbits(30) << 64) + (M64 + 1 - lo) % (M64 + 1)))    # the low halves sum to 2^64 or 0
    got = ask(["a %x %x %x %x" % (halves(a) + halves(b)) for a, b in pairs])
    for (a, b), g in zip(pairs, got):
        assert g == "%016x %016x" % halves(a + b), (a, b, g)
