"""How long the tap loads of the two-stage warp (csrc/lk_body_warp.h) stay in flight, read from an ISA listing (hipcc -S --cuda-device-only).
usage: python tools/isa_waits.py file.s <kernel name substring> [--min-valu N] [--all] [--cold]

A tap group is 8 buffer_load_dword through ONE resource with the scalar offset 0 and no immediate offset ("vN, vM, s[a:b], 0 offen"),
with no other vector-memory instruction between them: what warp_row_prepare issues.  (The rows of the march take their row offset
as the scalar offset, the old flow is wider, so nothing else in the march looks like that.)
From a group's last load the tool walks the kernel's control flow -- every branch both ways, except a branch on a flag that the path
itself has set (covering_waits) -- and counts on each path the vector-memory
instructions issued from the group's first load on (its own eight included; loads AND stores: gfx9 counts both in vmcnt, and they
complete in order) and the VALU instructions after its last.  A wait COVERS the group when its vmcnt is smaller than that number of
vector-memory instructions: the wave cannot go on before at least the group's first tap has landed (vmcnt(2) right behind the eight
loads holds it for six of them).  Per group it prints the covering wait that is nearest in VALU instructions, and with --all every covering
wait that some path meets first.  A path ends where it leaves the group's loop.  The listing cannot tell how often a branch is taken,
and a march has paths it takes a bounded number of times (priming, the second march's start, the drain) on which a wait right behind
the taps is the design: the source marks those blocks with a comment ("ofx-cold", csrc/lk_body_pair.h) and a path ends at such a
block too, unless --cold is given.  A listing without marks (the stream kernel's, a parent commit's) is walked on every path.
--min-valu N: exit status 1 when a group inside a loop is covered after fewer than N VALU instructions on some path."""
import heapq, re, sys

TAP = re.compile(r"^buffer_load_dword v\d+, v\d+, (s\[\d+:\d+\]), 0 offen$")
VMEM = ("buffer_", "global_", "flat_", "scratch_")
LABEL = re.compile(r"^\.L(BB\d+_\d+):")
VMCNT = re.compile(r"vmcnt\((\d+)\)")
COLD = "ofx-cold"  # csrc/lk_body_pair.h OFX_COLD_PATH(): a comment the source leaves in blocks a march runs a bounded number of times


def parse(lines, name):
    """The instructions of kernel `name`: list of (line number, text, loop header or None, block is marked cold), and label -> index."""
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and ":" in l and name in l.split(":")[0])
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    ins, labels, loop, block, cold = [], {}, None, 0, set()
    for n in range(start + 1, end + 1):
        l = lines[n]
        m = LABEL.match(l)
        if m or l.startswith("; %bb."):
            k = n + 1  # (a header inside another loop: "Parent Loop ..." here, "=>This Inner Loop Header: Depth=2" on a line below)
            while k <= end and lines[k].startswith("    ") and lines[k].lstrip().startswith(";"):
                l, k = l + lines[k], k + 1
            head = re.search(r"Loop Header: Depth=(\d+)", l)
            inside = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", l)
            loop = (m.group(1), int(head.group(1))) if (m and head) else ((inside.group(1), int(inside.group(2))) if inside else None)
            block += 1
            if m:
                labels[m.group(1)] = len(ins)
            continue
        t = l.strip()
        if COLD in t:
            cold.add(block)
        if not t or t[0] in ";.":
            continue
        ins.append((n + 1, t.split(";")[0].strip(), loop, block))
    return [(n, t, lp, b in cold) for n, t, lp, b in ins], labels


def groups(ins):
    """(index of first load, index of last load, resource) of every tap group."""
    out, run = [], []
    for i, (_, t, _, _) in enumerate(ins):
        m = TAP.match(t)
        if m and (not run or ins[run[0]][1].split(", ")[2] == m.group(1)):
            run.append(i)
            if len(run) == 8:
                out.append((run[0], run[-1], m.group(1)))
                run = []
        elif t.startswith(VMEM):
            run = [i] if m else []
    return out


FLAG_SET = re.compile(r"^s_mov_b64 (s\[\d+:\d+\]), (0|-1)$")
FLAG_TEST = re.compile(r"^s_(and|andn2)_b64 vcc, exec, (s\[\d+:\d+\])$")
SREG = re.compile(r"^s\[(\d+):(\d+)\]$|^s(\d+)$")


def sregs(operand):
    """The scalar registers an operand names."""
    m = SREG.match(operand)
    if not m:
        return set()
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m.group(1) else {int(m.group(3))}


def covering_waits(ins, labels, last, cold=False):
    """{index of wait: (VALU after the group's last load, vector-memory instructions from its first on) on the shortest path that meets it first}.
    hipcc turns `if (c) A else B; if (d) C` into blocks that leave a flag in a scalar register pair (s_mov_b64 s[a:b], 0 / -1) and branch
    on it again behind the join (s_and_b64 / s_andn2_b64 vcc, exec, s[a:b]; s_cbranch_vccz / vccnz).  A walk that took both ways there
    would join the tail of a cold path to a hot one, so the flags a path has set are part of its state (exec is taken as not 0)."""
    found, seen, heap, tick = {}, set(), [(0, 8, 0, last + 1, (), None)], 0
    while heap:
        valu, vm, _, i, flags, vcc = heapq.heappop(heap)  # flags: ((pair, value), ...); vcc: True (not 0) / False (0) / None
        while i < len(ins) and (i, vm, flags, vcc) not in seen:
            seen.add((i, vm, flags, vcc))
            if ins[last][2] and ins[i][2] != ins[last][2]:
                break  # the path leaves the group's loop: the march is over
            if ins[i][3] and not cold:
                break  # a block the source marks as run a bounded number of times per march
            t = ins[i][1]
            op = t.split()[0]
            ops = [o.strip() for o in t[len(op):].split(",")]
            if op == "s_waitcnt":
                m = VMCNT.search(t)
                if m and int(m.group(1)) < vm:
                    found.setdefault(i, (valu, vm))
                    break
            elif op == "s_endpgm":
                break
            elif op == "s_branch" or op.startswith("s_cbranch"):
                taken, falls = True, op != "s_branch"
                if op in ("s_cbranch_vccz", "s_cbranch_vccnz") and vcc is not None:
                    taken = vcc == (op == "s_cbranch_vccnz")
                    falls = not taken
                if taken:
                    tick += 1
                    heapq.heappush(heap, (valu, vm, tick, labels[ops[0][2:]], flags, vcc))
                if not falls:
                    break
            else:
                if op.startswith(VMEM):
                    vm = min(vm + 1, 64)
                elif op.startswith("v_"):
                    valu += 1
                ft = FLAG_TEST.match(t)
                if ft:
                    known = dict(flags).get(ft.group(2))
                    vcc = None if known is None else (known == -1) == (ft.group(1) == "and")
                elif "vcc" in t:
                    vcc = None
                written = sregs(ops[0]) if op.startswith(("s_", "v_cmp", "v_readfirstlane", "v_readlane")) and not op.startswith(("s_cmp", "s_bitcmp")) else set()
                if len(ops) > 1 and op.startswith("v_") and op.endswith(("_co_u32_e64", "_co_u32_e32", "_e64")) and sregs(ops[1]):
                    written |= sregs(ops[1])  # (carry-out / div_scale style second destinations)
                if written:
                    flags = tuple((p, v) for p, v in flags if not (sregs(p) & written))
                fs = FLAG_SET.match(t)
                if fs:
                    flags = tuple(sorted(dict(flags, **{fs.group(1): int(fs.group(2))}).items()))
            i += 1
    return found


def report(path, name, min_valu=None, show_all=False, cold=False, out=sys.stdout):
    ins, labels = parse(open(path).read().split("\n"), name)
    bad = 0
    for first, last, rs in groups(ins):
        loop = ins[first][2]
        found = covering_waits(ins, labels, last, cold)
        where = f"loop {loop[0]} depth {loop[1]}" if loop else "no loop"
        if not found:
            print(f"taps line {ins[first][0]} ({where}, {rs}): never covered", file=out)
            continue
        order = sorted(found.items(), key=lambda kv: kv[1])
        w, (valu, vm) = order[0]
        flag = ""
        if min_valu is not None and loop and valu < min_valu:
            bad += 1
            flag = "  << covered too soon"
        print(f"taps line {ins[first][0]} ({where}, {rs}): nearest cover after {valu} VALU, {vm - 8} vmem: line {ins[w][0]} {ins[w][1]}{flag}", file=out)
        if show_all:
            for w, (valu, vm) in order[1:]:
                print(f"      also after {valu} VALU, {vm - 8} vmem: line {ins[w][0]} {ins[w][1]}", file=out)
    return bad


if __name__ == "__main__":
    args = sys.argv[1:]
    mv = None
    if "--min-valu" in args:
        k = args.index("--min-valu")
        mv = int(args[k + 1])
        del args[k:k + 2]
    show_all, cold = "--all" in args, "--cold" in args
    args = [a for a in args if a not in ("--all", "--cold")]
    sys.exit(1 if report(args[0], args[1], mv, show_all, cold) else 0)
