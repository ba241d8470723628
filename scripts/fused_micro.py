"""Micro-benchmark of the m-space operator A*(B*q) (hgm_spmv_ab) at a BASELINE geometry: the
one-pass kernel (fused.hip) against the two SpMVs.  Prints one JSON line per variant.  Run on the
GPU box:
    python scripts/fused_micro.py [N angles reps [variants]]
Variants (comma-separated): `two` (the two SpMVs, the reference of the deviations) or
[w4]r<region>[q<0|4>][s<0-3>][v<2|3>]: the one pass (four waves) with that region side (fused_wregion), row pairs
(fused_rowpair, default 4), compact value stream mode (fused_vstream, default 1) and the compact
pass's ring depth (fused_vsdepth, default 3).  The other variants this script once timed (the
sub-chunk pass, wave / batch / depth shapes, fp32 accumulations, phase skips) are retired with
their kernels; DESIGN.md §3.5 keeps their measurements.
HGM_MICRO_F32=1: the fp32 operator (BASELINE configs[4]; the fp32 one-pass kernel)."""
import ctypes as C
import json
import re
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hybrid-gmres_amd"), ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401
import hgmres  # noqa: E402
from hgmres import _lib as L  # noqa: E402

N, na, reps = (int(a) for a in (sys.argv[1:4] if len(sys.argv) > 3 else (4096, 47, 20)))
variants = sys.argv[4].split(",") if len(sys.argv) > 4 else ["two", "r32", "r32q0", "r32s0", "r32v2"]


def variant_options(vname):
    mw = re.fullmatch(r"(?:w4)?r(\d+)(?:q([04]))?(?:s([0-3]))?(?:v([23]))?", vname)
    if vname == "two":
        return dict(fused_ab=0)
    if not mw:
        sys.exit(f"fused_micro: unknown variant {vname!r}: two, or [w4]r<region>[q<0|4>][s<0-3>][v<2|3>] "
                 "(the other variants are retired: DESIGN.md §3.5)")
    o = dict(fused_ab=1, fused_wregion=int(mw.group(1)))
    for name, val in (("fused_rowpair", mw.group(2)), ("fused_vstream", mw.group(3)), ("fused_vsdepth", mw.group(4))):
        if val is not None:
            o[name] = int(val)
    return o


options = [variant_options(v) for v in variants]      # (a typo fails before anything runs)
ctx = hgmres.Context(0)
lib = L.load()
f32 = os.environ.get("HGM_MICRO_F32", "0") == "1"
A = hgmres.SparseOperator.siddon(N, na, ctx=ctx, dtype=L.HGM_F32 if f32 else L.HGM_F64)
B = A.T
m, n = A.shape
dev = torch.device("cuda", 0)
tdt = torch.float32 if f32 else torch.float64
q = torch.from_numpy(np.random.default_rng(0).standard_normal(m)).to(dev).to(tdt)
bq = torch.empty(n, dtype=tdt, device=dev)
abq = torch.empty(m, dtype=tdt, device=dev)
P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
s_ = 4.0 if f32 else 8.0
two = 2 * (s_ + 4) * A.nnz + 8.0 * (m + 1) + 8.0 * (n + 1) + 2 * s_ * (m + n)
ref = None
for vname, o in zip(variants, options):
    with ctx.options(**o):
        lib.hgm_spmv_ab(ctx.handle, A._h, B._h, P(q), P(bq), P(abq))      # plan / warm-up
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            rc = lib.hgm_spmv_ab(ctx.handle, A._h, B._h, P(q), P(bq), P(abq))
        ctx.synchronize()
        dt = (time.perf_counter() - t0) / reps
    assert rc == 0
    out = abq.cpu().numpy()
    if vname == "two":
        ref = (bq.cpu().numpy(), out)
    dev_ = None if ref is None else float(np.linalg.norm(out - ref[1]) / np.linalg.norm(ref[1]))
    devz = None if ref is None else float(np.linalg.norm(bq.cpu().numpy() - ref[0]) / np.linalg.norm(ref[0]))
    print(json.dumps({"variant": vname, "N": N, "angles": na, "dtype": "f32" if f32 else "f64", "ms": round(dt * 1e3, 4),
                      "effective_GBps_two_pass": round(two / dt / 1e9, 1), "rel_dev_vs_two_pass": dev_, "bq_rel_dev": devz}), flush=True)
