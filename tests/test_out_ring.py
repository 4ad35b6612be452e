"""The ring descriptor of the stream pipeline's output stages (csrc/out_ring.h) on the host: tools/out_ring_main.cpp is built with the
host compiler and its slot index and window test are checked against the rule as include/ofx.h states it -- pair p goes to slot
(p - 1) mod slots, and a ring holds the newest `slots` pairs -- transcribed below, for every ring size, newest pair and pair asked
for that a short stream meets, the pairs just outside the window included; the index of every pair from 1 on, held or not.  No GPU.

tests/test_gpu_output_rings.py runs all five stages of a real session side by side on rings of different sizes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = range(1, 10)
NEWEST = range(0, 41)


def index(slots, pair):
    return (pair - 1) % slots


def holds(slots, newest, pair):
    return 1 <= pair <= newest and pair > newest - slots


@pytest.fixture(scope="module")
def ring(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("out_ring") / "out_ring_main")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "cuda_optical_flow_2_amd", "csrc"),
                           os.path.join(ROOT, "tools", "out_ring_main.cpp"), "-o", exe])

    def run(triples):
        args = [str(v) for t in triples for v in t]
        rows = [l.split() for l in subprocess.check_output([exe] + args, text=True).split("\n") if l]
        assert [tuple(map(int, r[:3])) for r in rows] == list(triples)
        return [(None if r[3] == "-" else int(r[3]), bool(int(r[4]))) for r in rows]
    return run


@pytest.mark.parametrize("slots", SLOTS)
def test_index_and_window_equal_the_rule(ring, slots):
    triples = [(slots, newest, pair) for newest in NEWEST for pair in range(-1, newest + 3)]
    got = ring(triples)
    inside = 0
    for (_, newest, pair), (idx, held) in zip(triples, got):
        what = f"slots {slots} newest {newest} pair {pair}"
        assert held == holds(slots, newest, pair), what
        assert idx == (index(slots, pair) if pair >= 1 else None), what   # (the program prints no index for a pair below 1: see there)
        inside += held
    assert inside == sum(min(slots, newest) for newest in NEWEST)   # (every window is as long as the ring, or the stream so far)


def test_the_pairs_a_ring_holds_have_distinct_slots(ring):
    for slots in SLOTS:
        for newest in (slots, 2 * slots + 1, 40):
            held = [idx for idx, h in ring([(slots, newest, pair) for pair in range(1, newest + 1)]) if h]
            assert sorted(held) == list(range(min(slots, newest))), f"slots {slots} newest {newest}"


def test_a_ring_without_slots_is_refused(ring):
    with pytest.raises(subprocess.CalledProcessError):
        ring([(0, 3, 1)])
