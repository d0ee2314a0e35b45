"""Many small LPs: BatchedDeviceHSD against the same LPs one after another on one analysed handle.

Inputs: B in {1, 8, 64, 512} copies of tests/golden/stair25.mps with seeded perturbations of the cost vector only (feasibility is untouched; the
sign of a column's perturbation follows its bounds, so the copies stay dual feasible too and every one has an optimum).
  batched     the B copies stacked into one handle and solved by BatchedDeviceHSD.optimize()
  sequential  the same LPs one after another through DeviceHSD.reload(c=...) + optimize() on ONE analysed handle (the best path without the
              batch); same process, same GPU
Median of three runs each.  Per B, written to profiles/hsd_batch_bench.json (also printed line by line): LPs per second both ways, wall time
per interior-point iteration (batched: per iteration of the batch, i.e. of its slowest LP), launches_update / launches_solve of both handles,
iterations per LP, statuses, and the largest relative difference of the objectives between the two ways.
Every batch size runs in a child process of its own under `timeout`; the driver stops at the first one that fails.

--skip-parked 0 runs the batch with every block factorised and swept (the default, and the behaviour before tlpk_ipm_batch_skip); 1 skips parked blocks.
tools/batch_skip_bench.py measures both settings side by side in one process.

    python tools/hsd_batch_bench.py [--sizes 1,8,64,512] [--reps 3] [--system K1] [--skip-parked 0]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT_S = {1: 120, 8: 120, 64: 180, 512: 420}          # per child process: analysis of the stack + 2 x reps solves of B LPs


def costs(d, B, seed=20261018, rel=0.01):
    """B seeded perturbations of the cost vector that keep the LP dual feasible (it stays primal feasible anyway, so every copy has an optimum):
    up on a column with a lower bound only, down with an upper bound only, either way on a boxed column, none on a free one."""
    lf, uf = np.isfinite(d.l), np.isfinite(d.u)
    scale = rel * np.maximum(np.abs(d.c), np.abs(d.c).mean())
    out = []
    for k in range(B):
        rng = np.random.default_rng(seed + k)
        up, both = rng.uniform(0.0, 1.0, d.c.shape[0]), rng.uniform(-1.0, 1.0, d.c.shape[0])
        out.append(d.c + scale * np.where(lf & uf, both, np.where(lf, up, np.where(uf, -up, 0.0))))
    return out


def worker(B, reps, system, skip=0):
    from tulip_jl_amd.hsd_batch import BatchedDeviceHSD
    from tulip_jl_amd.hsd_device import DeviceHSD
    from tulip_jl_amd.problem import read_free_mps, standard_form
    d = standard_form(read_free_mps(os.path.join(ROOT, "tests", "golden", "stair25.mps")))
    cs = costs(d, B)
    out = {"B": B, "system": system, "m": int(d.A.shape[0]), "n": int(d.A.shape[1]), "nnzA": int(d.A.nnz), "reps": reps, "skip_parked": int(skip)}
    med = lambda v: float(np.median(np.asarray(v, dtype=float)))                         # noqa: E731
    # batched
    t0 = time.perf_counter()
    opt = BatchedDeviceHSD([(d.A, d.b, c, d.l, d.u, d.c0, d.objsense) for c in cs], system=system, device=0, skip_parked=bool(skip))
    out["batched_setup_s"] = time.perf_counter() - t0
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        opt.optimize()
        wall.append(time.perf_counter() - t0)
    st = opt.kkt.stats()
    zb = opt.primal_objective.copy()
    iters = opt.niter.astype(int)
    out.update(batched_s=med(wall), batched_lps_per_s=B / med(wall), batched_ms_per_iteration=1e3 * med(wall) / int(iters.max()),
               batched_iterations_min=int(iters.min()), batched_iterations_max=int(iters.max()), batched_iterations_mean=float(iters.mean()),
               batched_status={s: int((opt.status == s).sum()) for s in set(opt.status.tolist())},
               batched_launches_update=int(st["launches_update"]), batched_launches_solve=int(st["launches_solve"]),
               batched_n_bump=int(opt.timers["n_bump"].sum()))
    opt.kkt.close()
    # sequential on one analysed handle
    t0 = time.perf_counter()
    one = DeviceHSD(d.A, d.b, cs[0], d.l, d.u, c0=d.c0, objsense_min=d.objsense, system=system, device=0)
    out["sequential_setup_s"] = time.perf_counter() - t0
    wall = []
    for _ in range(reps):
        zs, its, status = np.zeros(B), np.zeros(B, dtype=int), []
        t0 = time.perf_counter()
        for k in range(B):
            one.reload(c=cs[k]).optimize()
            zs[k], its[k] = one.primal_objective, one.niter
            status.append(one.status)
        wall.append(time.perf_counter() - t0)
    st = one.kkt.stats()
    out.update(sequential_s=med(wall), sequential_lps_per_s=B / med(wall), sequential_ms_per_iteration=1e3 * med(wall) / int(its.sum()),
               sequential_iterations_min=int(its.min()), sequential_iterations_max=int(its.max()), sequential_iterations_mean=float(its.mean()),
               sequential_status={s: status.count(s) for s in set(status)},
               sequential_launches_update=int(st["launches_update"]), sequential_launches_solve=int(st["launches_solve"]))
    one.kkt.close()
    out["speedup_lps_per_s"] = out["batched_lps_per_s"] / out["sequential_lps_per_s"]
    out["objective_max_rel_diff"] = float(np.max(np.abs(zb - zs) / (1 + np.abs(zs))))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,64,512")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--system", default="K1")
    ap.add_argument("--worker", type=int, default=0)
    ap.add_argument("--skip-parked", type=int, choices=[0, 1], default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hsd_batch_bench.json"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.reps, a.system, a.skip_parked)
    res = []
    for B in (int(s) for s in a.sizes.split(",")):
        limit = LIMIT_S.get(B, 420)
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--worker", str(B), "--reps", str(a.reps),
                            "--system", a.system, "--skip-parked", str(a.skip_parked)], capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"B = {B}: exit status {p.returncode}; nothing more is started on the GPU\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}", flush=True)
            break
        res.append(json.loads(line[0][len("RESULT "):]))
        print(json.dumps(res[-1]), flush=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/hsd_batch_bench.py", "results": res}, f, indent=1)
    return 0 if len(res) == len(a.sizes.split(",")) else 1


if __name__ == "__main__":
    sys.exit(main())
