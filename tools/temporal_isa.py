#!/usr/bin/env python3
"""Instruction counts of the temporal noise filter's kernels (csrc/temporal.hip) by issue class, from a listing made with the build's
own flags.

  python tools/temporal_isa.py          (needs hipcc only; no GPU)

Per kernel (temporal_filter_kernel<1> and <16>; each holds BOTH the C = 1 and the C = 3 path and both tap paths, so the counts
are of the whole kernel, not of what one wave executes): registers, scratch, occupancy, and the static number of vector, scalar,
vector-memory and LDS instructions, v_dot4_u32_u8, v_sad_u8 and the quarter-rate v_mul_lo_u32, and the global loads by width.
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from cuda_optical_flow_2_amd import build

    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "temporal.s")
        subprocess.run([build.hipcc()] + build.FLAGS + ["-S", "--cuda-device-only", "-o", out, os.path.join(build.CSRC, "temporal.hip")],
                       check=True, stderr=subprocess.DEVNULL)
        lines = open(out).read().split("\n")
    print("# python tools/temporal_isa.py")
    starts = [i for i, l in enumerate(lines) if l.startswith("_Z") and "temporal_filter_kernel" in l and ": ;" in l]
    for s in starts:
        end = next(i for i in range(s, len(lines)) if "s_endpgm" in lines[i])
        name = re.search(r"temporal_filter_kernelILi(\d+)E", lines[s]).group(1)
        h = collections.Counter()
        for l in lines[s:end]:
            m = re.match(r"\s+([a-z][a-z_0-9]+)\s", l)
            if m:
                h[m.group(1)] += 1
        info = {}
        for l in lines[end:end + 800]:
            m = re.match(r";\s*(NumVgprs|NumAgprs|TotalNumSgprs|ScratchSize|Occupancy|LDSByteSize):\s*(\d+)", l.strip())
            if m:
                info.setdefault(m.group(1), int(m.group(2)))
        cls = lambda p: sum(c for k, c in h.items() if k.startswith(p))
        print(f"temporal_filter_kernel<{name}>: " + ", ".join(f"{k} {v}" for k, v in info.items()))
        print(f"  vector {cls('v_')}, scalar {cls('s_')}, vector memory {cls('global_')}, LDS {cls('ds_')}")
        print(f"  v_dot4_u32_u8 {h['v_dot4_u32_u8']} (12 per pixel in grey, 36 in colour, four pixels each), v_sad_u8 {h['v_sad_u8']} "
              f"(3 and 9), v_alignbyte_b32 {h['v_alignbyte_b32']}, v_mul_lo_u32 {h['v_mul_lo_u32']}")
        print("  global loads: " + ", ".join(f"{k[12:]} {c}" for k, c in sorted(h.items()) if k.startswith("global_load_")))


if __name__ == "__main__":
    main()
