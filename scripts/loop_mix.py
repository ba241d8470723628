"""The main loop of kernels in a device assembly file (hipcc --cuda-device-only -S), by class.

usage: loop_mix.py FILE.s BATCHES SUBSTRING [SUBSTRING ...]   -- every function whose demangled
name contains all substrings: its main loop (the backward branch around the LDS adds), the instruction
counts of one trip by class (SALU, VALU, LDS, VMEM, s_waitcnt, branch) and per batch (a trip holds
BATCHES batches: the ring depth of k_fused_rw), the v_add_u32 / v_readlane / v_cndmask counts of
the trip, and the order of the LDS reads (R), the lgkmcnt waits [n], the vmcnt waits {n} and the
accumulator adds (A, runs counted).  Also: the waits before the kernel's first ds_read."""
import re
import subprocess
import sys
from collections import Counter

from asm_mix import functions


def klass(op):
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "VMEM"
    return "VALU"


def order(ins):
    out, adds = [], 0
    for i in ins:
        op = i.split()[0]
        if op.startswith("ds_add"):
            adds += 1
            continue
        if adds:
            out.append(f"A{adds} ")
            adds = 0
        if op.startswith("ds_read"):
            out.append("R")
        elif op == "s_waitcnt":
            out += [f"[{n}]" for n in re.findall(r"lgkmcnt\((\d+)\)", i)]
            out += [f"{{{n}}}" for n in re.findall(r"vmcnt\((\d+)\)", i)]
    if adds:
        out.append(f"A{adds} ")
    return "".join(out)


def main():
    path, nb, subs = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    for name, body in functions(path):
        dm = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        if not all(x in dm for x in subs):
            continue
        lines = body.split("\n")
        label, ins = {}, []
        for ln in lines:
            m = re.match(r"(\.LBB\d+_\d+):", ln)
            if m:
                label[m.group(1)] = len(ins)
            elif ln.startswith("\t") and not ln.strip().startswith((".", ";")):
                ins.append(ln.strip().split(";")[0].strip())
        # the main loop: the backward branch whose span holds the most accumulator adds (the
        # shortest such span; without LDS adds: the most LDS instructions)
        what = "ds_add" if any(s.startswith("ds_add") for s in ins) else "ds_"
        best, score = (0, 0), (-1, 0)
        for i, s in enumerate(ins):
            m = re.match(r"s_cbranch\w+\s+(\.LBB\d+_\d+)", s)
            if m and label.get(m.group(1), i + 1) <= i:
                a = label[m.group(1)]
                sc = (sum(t.startswith(what) for t in ins[a:i + 1]), a - i)
                if sc > score:
                    best, score = (a, i + 1), sc
        loop = ins[best[0]:best[1]]
        c = Counter(klass(i.split()[0]) for i in loop)
        ops = Counter(i.split()[0] for i in loop)
        first = next((k for k, s in enumerate(ins) if s.startswith("ds_read")), len(ins))
        early = [s for s in ins[:first] if s.startswith("s_waitcnt")]
        print(re.search(r"k_\w+<[^>]*>|k_\w+", dm).group(0))
        print(f"  kernel {len(ins)} instructions; main loop {len(loop)} per trip ({nb} batches), {len(loop) / nb:.1f} per batch: "
              + " ".join(f"{k} {c[k]}" for k in ("SALU", "VALU", "LDS", "VMEM", "s_waitcnt", "branch")))
        print("  in the loop: " + " ".join(f"{k} {ops[k]}" for k in ("v_add_u32_e32", "v_readlane_b32", "v_cndmask_b32_e64",
                                                                     "v_cndmask_b32_e32", "s_cselect_b32", "s_cselect_b64")))
        print("  loop order: " + order(loop))
        print(f"  waits before the first ds_read ({len(early)}): " + " ".join(s.split(None, 1)[1] for s in early))


if __name__ == "__main__":
    main()
