#!/usr/bin/env python3
"""One line per (unit, kernel) of the library's device code: name, body hash, descriptor hash.

Compiles every .hip unit of a csrc directory with the Makefile's flags plus
`--cuda-device-only -S` (unit id pinned with -cuid=, which otherwise hashes the source path into a
symbol name) and hashes, per kernel symbol, its instructions (comments dropped, the function number
of local labels dropped: emission order may differ between two trees) and its
.amdhsa_kernel ... .end_amdhsa_kernel block (registers, LDS, scratch).  Two trees carry the same
device code when their listings are equal.  --brief prints one line per unit instead: the unit, its
kernel count and the sha256 of its per-kernel lines (what profiles/ keeps).  --anonymous compares
trees whose kernels were renamed (other template parameters, the same instructions): each kernel is
hashed with its own symbol replaced by a fixed token and the lines are printed sorted, without names:

    python scripts/kernel_listing.py hybrid-gmres_amd/csrc > branch.txt
    python scripts/kernel_listing.py ../parent/hybrid-gmres_amd/csrc > parent.txt && cmp parent.txt branch.txt
"""
import argparse
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ("-O3 -std=c++17 -fPIC -fvisibility=hidden -ffp-contract=off --offload-arch=gfx950 "
         "-Wall -Wno-unused-function -Wno-unused-result").split()
LOCAL = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI)\d+(_\d+)?")


def assembly(csrc, unit, extra, tmp):
    out = os.path.join(tmp, unit + ".s")
    hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    inc = ["-I" + os.path.join(csrc, "..", "..", "include"), "-I" + csrc]
    subprocess.run([hipcc, *FLAGS, *inc, *extra, "-cuid=listing", "--cuda-device-only", "-S", "-x", "hip",
                    os.path.join(csrc, unit), "-o", out], check=True)
    with open(out) as f:
        return f.read().splitlines()


def normal(lines):
    keep = []
    for ln in lines:
        ln = ln.split(";", 1)[0].rstrip()
        if ln:
            keep.append(LOCAL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), ln))
    return hashlib.sha256("\n".join(keep).encode()).hexdigest()[:16]


def kernels(lines, anonymous=False):
    """{kernel: (body hash, descriptor hash)} of one unit's assembly; anonymous: with the kernel's own
    symbol (the .size / .set lines of the body, the .amdhsa_kernel line) replaced by a fixed token"""
    start = {}
    for i, ln in enumerate(lines):
        m = re.match(r"([A-Za-z_][\w.$]*):", ln)
        if m:
            start.setdefault(m.group(1), i)
    found = {}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            j = i
            while not lines[j].strip().startswith(".end_amdhsa_kernel"):
                j += 1
            name = m.group(1)
            body = [ln for ln in lines[start[name] + 1:i] if not re.match(r"\s*\.(section|p2align)\b", ln)]
            desc = lines[i:j + 1]
            if anonymous:
                own = re.compile(r"(?<![\w.$])" + re.escape(name) + r"(?![\w$])")
                body, desc = ([own.sub("KERNEL", ln) for ln in part] for part in (body, desc))
            found[name] = (normal(body), normal(desc))
            i = j
        i += 1
    return found


def brief(listing):
    """one line per unit of a per-kernel listing: unit, kernel count, sha256 of its lines"""
    units = {}
    for ln in listing:
        units.setdefault(ln.split(" ", 1)[0], []).append(ln)
    return [f"{u} {len(ls)} {hashlib.sha256(chr(10).join(ls).encode()).hexdigest()}" for u, ls in units.items()]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("csrc")
    ap.add_argument("--units", nargs="*", help="default: every .hip of the directory")
    ap.add_argument("--extra", default="", help="further compiler flags, e.g. -DHGM_EXPERIMENTS=1")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--brief", action="store_true", help="one line per unit: kernel count and hash of its lines")
    ap.add_argument("--anonymous", action="store_true",
                    help="hash each kernel without its own symbol and list sorted (unit, body, descriptor) lines "
                         "without names: equal multisets = the same kernels under other names")
    a = ap.parse_args()
    units = a.units or sorted(u for u in os.listdir(a.csrc) if u.endswith(".hip"))
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        texts = list(pool.map(lambda u: assembly(a.csrc, u, a.extra.split(), tmp), units))
    if a.anonymous:
        listing = sorted(f"{unit} {body} {desc}" for unit, lines in zip(units, texts)
                         for body, desc in kernels(lines, True).values())
    else:
        listing = [f"{unit} {name} {body} {desc}" for unit, lines in zip(units, texts)
                   for name, (body, desc) in sorted(kernels(lines).items())]
    print("\n".join(brief(listing) if a.brief else listing))


if __name__ == "__main__":
    sys.exit(main())
