"""tools/isa_waits.py on two hand-written listings (tests/golden/isa_waits_*.s): no compiler, no GPU.

drained: the eight taps are issued in a branch; behind the join the wait for an OLDER load is vmcnt(0), two VALU instructions after
the last tap -- what the fused iteration march did before its paths were made to wait for their own loads.
counted: the taps are followed by two row loads and a store; vmcnt(10) in front of them leaves all eight in flight (ten
vector-memory instructions were issued from the first tap on), vmcnt(3) eight VALU instructions later is the first wait that holds
the wave for them.  The step without taps is marked cold and leaves a flag; its unmarked tail behind the join drains everything
and is only reached with that flag."""
import importlib.util
import io
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "isa_waits.py")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _tool():
    spec = importlib.util.spec_from_file_location("isa_waits", TOOL)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _one_group(m, listing, kernel, cold=False):
    ins, labels = m.parse(open(os.path.join(GOLDEN, listing)).read().split("\n"), kernel)
    gs = m.groups(ins)
    assert len(gs) == 1 and gs[0][1] - gs[0][0] >= 7 and gs[0][2] == "s[12:15]", gs
    assert ins[gs[0][0]][2] == ("BB0_1", 1), "the group lies in the loop"
    found = m.covering_waits(ins, labels, gs[0][1], cold)
    return {ins[w][1]: v for w, v in found.items()}


def test_drained_group():
    m = _tool()
    found = _one_group(m, "isa_waits_drained.s", "drained")
    assert found == {"s_waitcnt vmcnt(0)": (2, 8)}, found   # 2 VALU after the last tap; only the group's own 8 loads issued
    out = io.StringIO()
    assert m.report(os.path.join(GOLDEN, "isa_waits_drained.s"), "drained", min_valu=5, out=out) == 1
    assert "covered too soon" in out.getvalue() and "after 2 VALU, 0 vmem" in out.getvalue(), out.getvalue()
    assert m.report(os.path.join(GOLDEN, "isa_waits_drained.s"), "drained", min_valu=2, out=io.StringIO()) == 0


def test_counted_group():
    m = _tool()
    for cold in (False, True):   # (the cold step's own blocks are not reachable from the taps before the covering wait)
        found = _one_group(m, "isa_waits_counted.s", "counted", cold)
        assert found == {"s_waitcnt vmcnt(3)": (8, 11)}, found   # vmcnt(10) did not cover, the flagged tail was not walked
    assert m.report(os.path.join(GOLDEN, "isa_waits_counted.s"), "counted", min_valu=8, out=io.StringIO()) == 0
    assert m.report(os.path.join(GOLDEN, "isa_waits_counted.s"), "counted", min_valu=9, out=io.StringIO()) == 1


def test_command_line_exit_status():
    run = lambda *a: subprocess.run([sys.executable, TOOL, *a], capture_output=True, text=True)
    r = run(os.path.join(GOLDEN, "isa_waits_drained.s"), "drained", "--min-valu", "300")
    assert r.returncode == 1 and "taps line" in r.stdout, r.stdout + r.stderr
    r = run(os.path.join(GOLDEN, "isa_waits_counted.s"), "counted", "--min-valu", "8", "--all")
    assert r.returncode == 0 and "after 8 VALU, 3 vmem" in r.stdout, r.stdout + r.stderr
