"""Generator time of the unmatched fan-beam back-projector.  Run on an MI355X:
    python scripts/fan_backproj_micro.py [N] [n_angles] [reps]        default 4096 47 5
hgm_mat_create_fan_backprojector against hgm_mat_create_backprojector (the parallel-beam one) at the same size,
fp64, the tiled row order: both count their entries, scan, and fill 12 B per entry; the fan one adds an atan2, two
16-B table loads per side pair and a division per (pixel, source).

Each call is timed whole (count pass, scan, allocation, fill pass and the operator's finalisation: bands and the
streaming index) between two HIP events on the context's stream, next to the host clock; the two generators
alternate, each warmed once, median of `reps`.  One JSON line.  For the split between the two generator kernels and
the rest of a call run it once under `rocprofv3 --kernel-trace --stats`.
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hybrid-gmres_amd"), ROOT]
import torch  # noqa: E402
import hgmres  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
NA = int(sys.argv[2]) if len(sys.argv) > 2 else 47
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
ctx = hgmres.Context(0)
stream = torch.cuda.ExternalStream(int(ctx.stream()), device=torch.device("cuda", 0))


def timed(make):
    """(event ms, host ms, nnz) of one generator call; the operator is released before the next."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ctx.synchronize()
    t0 = time.perf_counter()
    e0.record(stream)
    M = make()
    e1.record(stream)
    e1.synchronize()
    host = (time.perf_counter() - t0) * 1e3
    nnz = M.nnz
    M.close()
    return e0.elapsed_time(e1), host, nnz


routes = {"fan": lambda: hgmres.SparseOperator.fan_backprojector(N, NA, ctx=ctx),
          "parallel": lambda: hgmres.SparseOperator.pixel_backprojector(N, NA, ctx=ctx)}
for make in routes.values():                                             # warm both
    timed(make)
ev = {k: [] for k in routes}
ho = {k: [] for k in routes}
nnz = {}
for _ in range(reps):                                                    # alternating
    for k, make in routes.items():
        e, h, nnz[k] = timed(make)
        ev[k].append(e)
        ho[k].append(h)
out = dict(what="fan vs parallel back-projector generator", N=N, n_angles=NA, reps=reps)
for k in routes:
    out[f"{k}_nnz"] = int(nnz[k])
    out[f"{k}_event_ms"] = round(statistics.median(ev[k]), 2)
    out[f"{k}_event_ms_min"] = round(min(ev[k]), 2)
    out[f"{k}_event_ms_max"] = round(max(ev[k]), 2)
    out[f"{k}_host_ms"] = round(statistics.median(ho[k]), 2)
out["fan_over_parallel"] = round(out["fan_event_ms"] / out["parallel_event_ms"], 3)
print(json.dumps(out), flush=True)
ctx.close()
del ctx
