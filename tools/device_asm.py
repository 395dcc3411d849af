#!/usr/bin/env python
"""Device listings of the HIP sources: what a host-only change to ppo_amd/csrc/ has to leave unchanged.

    python tools/device_asm.py record --root DIR --out DIR2   (CPU, hipcc cross-compiles)
    python tools/device_asm.py compare A B                    (CPU)

`record` compiles every ppo_amd/csrc/*.hip of the tree at DIR with the flags of ppo_amd/build.py plus
`--offload-device-only -S` into DIR2/<name>.s, so one copy of this tool records a checkout of another commit and this
tree.  `compare` cuts each listing into one piece per function symbol - its preamble, its code, a kernel's
.amdhsa_kernel descriptor block and the resource summary that follows - and pairs the pieces of A and B by symbol, so
the order in which the compiler emitted them does not matter; the labels that carry a function's ordinal (.LBB<n>_<m>,
.Lfunc_end<n>, .LJTI<n>_<m>, BB<n>_<m> in comments) are written without it, and the blanks that align the comment behind
a block label (as many as the ordinal's digits leave room for) as one.  Each kernel's entry under amdhsa.kernels is
compared with its piece, and what is left of the file (object definitions, section bookkeeping, the rest of the metadata)
as a sorted list of lines.  Only the lines that name the per-compilation `__hip_cuid_<hash>` symbol are left out.  The tool compares
text: it does not look for anything in a listing.  It prints `equal: N files, M kernels`, or the first differing symbol
per file, and exits non-zero on any difference.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ARCH = "gfx950"
ORDINAL = re.compile(r"(\.LBB|\.Lfunc_begin|\.Lfunc_end|\.LJTI|\bBB)\d+")  # BB<n>_<m>: the loop comments
LABEL_PAD = re.compile(r"^(\.LBB_\d+:)\s+;")  # the comment behind a block label is aligned by the label's width
BEGIN = re.compile(r"; -- Begin function (\S+)")
RESOURCE = re.compile(r"\t\.set |\t\.section\t\.AMDGPU\.csdata|;")  # what follows a function's end and belongs to it


def hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found")


def record(root, out):
    csrc = os.path.join(root, "ppo_amd", "csrc")
    os.makedirs(out, exist_ok=True)
    # ppo_amd/build.py's compile flags
    flags = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function",
             "-I", os.path.join(root, "include")]
    cc = hipcc()
    jobs = [[cc, *flags, "--offload-device-only", "-S", os.path.join(csrc, s), "-o", os.path.join(out, s[:-4] + ".s")]
            for s in sorted(os.listdir(csrc)) if s.endswith(".hip")]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(lambda cmd: subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL), jobs))
    print(f"recorded {len(jobs)} listings in {out}")


def split(path):
    """-> ({symbol: lines}, sorted rest, kernel count)"""
    with open(path) as f:
        lines = [LABEL_PAD.sub(r"\1 ;", ORDINAL.sub(r"\1", l.rstrip())) for l in f if "__hip_cuid_" not in l]
    meta_at = next((i for i, l in enumerate(lines) if l.strip() == ".amdgpu_metadata"), len(lines))
    pieces, rest = {}, []
    begins = [i for i in range(meta_at) if BEGIN.search(lines[i])]
    # a piece starts where the previous one ended (its .section / .text preamble goes with it), the first one after the
    # two target lines at the top of the file
    start = next((i for i, l in enumerate(lines) if not l.startswith(("\t.amdgcn_target", "\t.amdhsa_code_object_version"))), 0)
    rest += lines[:start]
    for b in begins:
        sym = BEGIN.search(lines[b]).group(1)
        end = next(i for i in range(b, meta_at) if lines[i].strip() == "; -- End function") + 1
        while end < meta_at and RESOURCE.match(lines[end]):
            end += 1
        assert sym not in pieces, f"{path}: {sym} defined twice"
        pieces[sym] = lines[start:end]
        start = end
    rest += lines[start:meta_at]
    # metadata: the entries of amdhsa.kernels go to their kernels, the remainder to the rest
    entries = []
    for l in lines[meta_at:]:
        if l.startswith("  - "):
            entries.append([l])
        elif entries and l.startswith("    "):
            entries[-1].append(l)
        else:
            entries.append([l])
    for e in entries:
        name = next((m.group(1) for m in (re.match(r"    \.name:\s+(\S+)", l) for l in e) if m), None)
        if name is None:
            rest += e
        else:
            pieces[name] = pieces[name] + ["; metadata entry"] + e  # KeyError: an entry without a function
    kernels = sum(1 for p in pieces.values() for l in p if l.startswith("\t.amdhsa_kernel "))
    return pieces, sorted(rest), kernels


def first_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return f"line {i}: {x.strip()!r} != {y.strip()!r}"
    return f"{len(a)} lines != {len(b)} lines"


def compare(dir_a, dir_b):
    names_a = sorted(f for f in os.listdir(dir_a) if f.endswith(".s"))
    names_b = sorted(f for f in os.listdir(dir_b) if f.endswith(".s"))
    bad, kernels = 0, 0
    for name in sorted(set(names_a) ^ set(names_b)):
        print(f"{name}: only in {dir_a if name in names_a else dir_b}")
        bad += 1
    for name in sorted(set(names_a) & set(names_b)):
        pa, ra, ka = split(os.path.join(dir_a, name))
        pb, rb, _ = split(os.path.join(dir_b, name))
        kernels += ka
        only = sorted(set(pa) ^ set(pb))
        if only:
            print(f"{name}: {only[0]} only in {dir_a if only[0] in pa else dir_b} ({len(only)} such symbols)")
            bad += 1
            continue
        diff = next((s for s in sorted(pa) if pa[s] != pb[s]), None)
        if diff:
            print(f"{name}: {diff}: {first_difference(pa[diff], pb[diff])}")
            bad += 1
        elif ra != rb:
            print(f"{name}: outside the functions: {first_difference(ra, rb)}")
            bad += 1
    if bad:
        print(f"different: {bad} of {len(set(names_a) | set(names_b))} files")
        return 1
    print(f"equal: {len(names_a)} files, {kernels} kernels")
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("record")
    r.add_argument("--root", required=True)
    r.add_argument("--out", required=True)
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    args = ap.parse_args()
    if args.cmd == "record":
        record(args.root, args.out)
        return 0
    return compare(args.a, args.b)


if __name__ == "__main__":
    sys.exit(main())
