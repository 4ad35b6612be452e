"""Instruction histogram of the LK march loops of one kernel in an ISA listing (hipcc -S --cuda-device-only).
usage: python tools/isa_loops.py file.s <kernel name substring> [unroll=3] [op=v_dot2c_i32_i16_e32]
Prints NumVgprs / scratch, then for every loop (of any depth; its own blocks only) that holds `op` (v_dot2c: the LK marches; v_min_f32_e32: the
flow median's quad march, unroll 1, one loop per radius): VALU / SALU / memory instructions per step (loop body / unroll),
split into the two issue classes of tools/ubench/valu_rates.hip (cheap: plain 32-bit add / sub / and / or / xor / mov / fp32 add, mul, fma;
full: everything else) and an estimate of the VALU time per step from the measured rates (1.15 / 1.85 ns, v_rcp_f64 6.85)."""
import collections, re, sys
path, name = sys.argv[1], sys.argv[2]
unroll = int(sys.argv[3]) if len(sys.argv) > 3 else 3
op = sys.argv[4] if len(sys.argv) > 4 else "v_dot2c_i32_i16_e32"
lines = open(path).read().split("\n")
start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and name in l.split(":")[0] and ":" in l)
end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
e2 = end
while "NumVgprs" not in lines[e2]:
    e2 += 1
for l in lines[e2 - 3:e2 + 14]:
    if re.search(r"NumVgprs|ScratchSize|Occupancy|TotalNumSgprs", l):
        print(l.strip())
body = lines[start:end]
# The blocks of every loop, by the annotations hipcc leaves on block labels ("=>This Inner Loop Header: Depth=2", "in Loop:
# Header=BB0_32 Depth=2"): a block counts for the innermost loop it is in, so the march nested in lk_pair_kernel's loop over a wave's
# segments (depth 2) is counted without the per-segment set-up around it, and a march of depth 1 without the kernel's tail.
loops, cur = collections.OrderedDict(), None
for l in body:
    if l.startswith(".LBB") or l.startswith("; %bb."):
        head = re.match(r"\.L(BB\d+_\d+):.*Loop Header: Depth=(\d+)", l)
        inside = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", l)
        cur = head.group(1) if head else (inside.group(1) if inside else None)
        if cur:
            loops.setdefault(cur, [int((head or inside).group(2)), []])
        continue
    if cur:
        loops[cur][1].append(l)
CHEAP = {"v_add_u32_e32", "v_sub_u32_e32", "v_subrev_u32_e32", "v_and_b32_e32", "v_or_b32_e32", "v_xor_b32_e32", "v_mov_b32_e32", "v_add_f32_e32", "v_sub_f32_e32",
         "v_mul_f32_e32", "v_fma_f32", "v_fmac_f32_e32", "v_add_u32_e64", "v_sub_u32_e64", "v_accvgpr_write_b32", "v_accvgpr_read_b32"}
for a, (depth, seg) in loops.items():
    ops = collections.Counter()
    for l in seg:
        l = l.strip()
        if not l or l.startswith(";") or l.startswith("."):
            continue
        ops[l.split()[0]] += 1
    if not ops[op]:
        continue
    valu = sum(c for o, c in ops.items() if o.startswith("v_"))
    cheap = sum(c for o, c in ops.items() if o in CHEAP)
    salu = sum(c for o, c in ops.items() if o.startswith("s_"))
    mem = sum(c for o, c in ops.items() if o.startswith(("buffer_", "global_", "scratch_", "ds_", "flat_")))
    ns = (cheap * 1.15 + (valu - cheap - ops["v_rcp_f64_e32"]) * 1.85 + ops["v_rcp_f64_e32"] * 6.85) / unroll
    print(f"loop {a} depth {depth}: per step VALU {valu/unroll:.0f} (cheap {cheap/unroll:.0f})  SALU {salu/unroll:.0f}  mem {mem/unroll:.1f}  scratch {sum(c for o,c in ops.items() if o.startswith('scratch_'))/unroll:.1f}  ~{ns:.0f} ns VALU")
    print("   " + "  ".join(f"{o}:{c/unroll:.1f}" for o, c in ops.most_common(28)))
