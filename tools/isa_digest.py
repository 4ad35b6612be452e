#!/usr/bin/env python3
"""One digest per GPU kernel of the default build, to prove that a source change left the device code alone.

    python tools/isa_digest.py --out before.txt        (on the old tree)
    python tools/isa_digest.py --out after.txt         (on the new tree)
    python tools/isa_digest.py --compare before.txt after.txt
    python tools/isa_digest.py --compare before.txt after.txt --rename REGEX REPL     (a kernel template lost or gained a parameter)

Every .hip unit of build.SOURCES is compiled with build.FLAGS plus --cuda-device-only -S.  A kernel's digest is the SHA-256 of its
assembly body, its .amdhsa_kernel block (registers, static LDS, occupancy attributes) and its metadata entry (arguments, limits),
with what depends on the compilation unit rather than on the kernel normalised away: the __hip_cuid_* symbol and the function index
inside local labels and block names, so that the order in which the kernels are emitted does not matter, and the kernel's own mangled
name (in its labels, its metadata and the symbols of its static LDS), so that a change of its template's parameter list alone leaves
the digest as it was; --rename then maps the old names to the new ones.  Digests only: nothing is searched for.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cuda_optical_flow_2_amd import build  # noqa: E402

# (the last two: block names inside comments -- "in Loop: Header=BB14_106" -- and the padding in front of a comment, which follows the
# length of the label before it)
NORMALISE = [(re.compile(r"__hip_cuid_[0-9a-f]+"), "__hip_cuid_"), (re.compile(r"\.L(BB|JTI)\d+_(\d+)"), r".L\1_\2"),
             (re.compile(r"\.Lfunc_(begin|end)\d+"), r".Lfunc_\1"), (re.compile(r"\bBB\d+_(\d+)"), r"BB_\1"), (re.compile(r"[ \t]+;"), " ;")]


def unit_digests(unit, tmp):
    asm = os.path.join(tmp, unit + ".s")
    cmd = [build.hipcc()] + build.FLAGS + ["--cuda-device-only", "-S", os.path.join(build.CSRC, unit), "-o", asm]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {unit}:\n{r.stderr}")
    with open(asm) as f:
        text = f.read()
    for rx, to in NORMALISE:
        text = rx.sub(to, text)
    meta = text[text.index("amdhsa.kernels:"):text.index("amdhsa.target:")] if "amdhsa.kernels:" in text else ""
    entries = {re.search(r"\.name:\s+(\S+)", e).group(1): e for e in re.split(r"\n(?=  - )", meta)[1:]}
    out = []
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n.*?^\t\.end_amdhsa_kernel$", text, re.S | re.M):
        name = m.group(1)
        body = re.search(r"^%s:.*?^\.Lfunc_end:" % re.escape(name), text, re.S | re.M).group(0)
        h = hashlib.sha256("\n".join([body, m.group(0), entries[name]]).replace(name[2:], "KERNEL").encode()).hexdigest()
        out.append(f"{unit} {name} {h}")
    return out


def read(path):
    with open(path) as f:
        return {tuple(l.split()[:2]): l.split()[2] for l in f if l.strip()}


def compare(a, b, rename=None):
    da, db = read(a), read(b)
    if rename:
        da = {(u, re.sub(rename[0], rename[1], k)): h for (u, k), h in da.items()}
    differ = sorted(k for k in da if k in db and da[k] != db[k])
    missing, extra = sorted(set(da) - set(db)), sorted(set(db) - set(da))
    for tag, ks in (("differs", differ), ("missing", missing), ("extra", extra)):
        for k in ks:
            print(tag, *k)
    print(f"{len(da)} kernels before, {len(db)} after: {len(differ)} differ, {len(missing)} missing, {len(extra)} extra")
    return 1 if differ or missing or extra else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="write the sorted 'unit kernel digest' lines here (default: stdout)")
    ap.add_argument("--compare", nargs=2, metavar=("BEFORE", "AFTER"), help="compare two such files")
    ap.add_argument("--rename", nargs=2, metavar=("REGEX", "REPL"), help="with --compare: re.sub applied to the kernel names of BEFORE")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare, rename=args.rename)
    units = [s for s in build.SOURCES if s.endswith(".hip")]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(os.cpu_count() or 4, 8)) as ex:
        lines = sorted(l for ls in ex.map(lambda u: unit_digests(u, tmp), units) for l in ls)
    with (open(args.out, "w") if args.out else sys.stdout) as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
