"""Many small LPs through Mehrotra's loop: BatchedDeviceMPC against the same LPs one after another, and against the HSD batch.

Inputs: those of tools/hsd_batch_bench.py -- B in {1, 8, 64, 512} copies of tests/golden/stair25.mps with seeded perturbations of the cost
vector (`costs` of that tool: every copy keeps an optimum).  In ONE process per B, on the same GPU:
  mpc_batched  the B copies stacked into one handle and solved by BatchedDeviceMPC.optimize()
  sequential   the same LPs one after another through DeviceMPC.reload(c=...) + optimize() on ONE analysed handle
  hsd_batched  the same stack through BatchedDeviceHSD.optimize() (the batch the project had before)
Median of `reps` runs each.  Per B, written to profiles/mpc_batch_bench.json (also printed line by line): LPs per second of the three, wall
time per interior-point iteration of the batch (i.e. of its slowest LP), iterations per LP (mean, and the batch's own = its slowest LP's),
statuses, and the largest relative difference of the objectives between the MPC batch and the sequential solves.
Every batch size runs in a child process of its own under `timeout`; the driver stops at the first one that fails.

    python tools/mpc_batch_bench.py [--sizes 1,8,64,512] [--reps 3] [--system K1]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIMIT_S = {1: 120, 8: 120, 64: 240, 512: 600}          # per child process: two analyses of the stack + 3 x reps solves of B LPs


def note(msg):
    print(msg, file=sys.stderr, flush=True)


def run_batch(cls, lps, system, reps, tag, skip=0):
    med = lambda v: float(np.median(np.asarray(v, dtype=float)))                         # noqa: E731
    B = len(lps)
    t0 = time.perf_counter()
    opt = cls(lps, system=system, device=0, skip_parked=bool(skip))
    out = {f"{tag}_setup_s": time.perf_counter() - t0}
    wall = []
    for r in range(reps):
        t0 = time.perf_counter()
        opt.optimize()
        wall.append(time.perf_counter() - t0)
        note(f"  B = {B} {tag} run {r}: {wall[-1]:.3f} s")
    iters = opt.niter.astype(int)
    out.update({f"{tag}_s": med(wall), f"{tag}_lps_per_s": B / med(wall), f"{tag}_ms_per_iteration": 1e3 * med(wall) / max(int(iters.max()), 1),
                f"{tag}_iterations_mean": float(iters.mean()), f"{tag}_iterations_min": int(iters.min()), f"{tag}_iterations_of_the_batch": int(iters.max()),
                f"{tag}_status": {s: int((opt.status == s).sum()) for s in set(opt.status.tolist())}, f"{tag}_n_bump": int(opt.timers["n_bump"].sum())})
    z = opt.primal_objective.copy()
    opt.kkt.close()
    return out, z


def worker(B, reps, system, skip=0):
    from hsd_batch_bench import costs
    from tulip_jl_amd.hsd_batch import BatchedDeviceHSD
    from tulip_jl_amd.mpc_batch import BatchedDeviceMPC
    from tulip_jl_amd.mpc_device import DeviceMPC
    from tulip_jl_amd.problem import read_free_mps, standard_form
    d = standard_form(read_free_mps(os.path.join(ROOT, "tests", "golden", "stair25.mps")))
    cs = costs(d, B)
    lps = [(d.A, d.b, c, d.l, d.u, d.c0, d.objsense) for c in cs]
    out = {"B": B, "system": system, "m": int(d.A.shape[0]), "n": int(d.A.shape[1]), "nnzA": int(d.A.nnz), "reps": reps, "skip_parked": int(skip)}
    med = lambda v: float(np.median(np.asarray(v, dtype=float)))                         # noqa: E731
    res, zb = run_batch(BatchedDeviceMPC, lps, system, reps, "mpc_batched", skip)
    out.update(res)
    # sequential on one analysed handle
    t0 = time.perf_counter()
    one = DeviceMPC(d.A, d.b, cs[0], d.l, d.u, c0=d.c0, objsense_min=d.objsense, system=system, device=0)
    out["sequential_setup_s"] = time.perf_counter() - t0
    wall = []
    for r in range(reps):
        zs, its, status = np.zeros(B), np.zeros(B, dtype=int), []
        t0 = time.perf_counter()
        for k in range(B):
            one.reload(c=cs[k]).optimize()
            zs[k], its[k] = one.primal_objective, one.niter
            status.append(one.status)
        wall.append(time.perf_counter() - t0)
        note(f"  B = {B} sequential run {r}: {wall[-1]:.3f} s")
    out.update(sequential_s=med(wall), sequential_lps_per_s=B / med(wall), sequential_ms_per_iteration=1e3 * med(wall) / max(int(its.sum()), 1),
               sequential_iterations_mean=float(its.mean()), sequential_iterations_min=int(its.min()), sequential_iterations_max=int(its.max()),
               sequential_status={s: status.count(s) for s in set(status)})
    one.kkt.close()
    res, zh = run_batch(BatchedDeviceHSD, lps, system, reps, "hsd_batched", skip)
    out.update(res)
    out["speedup_over_sequential"] = out["mpc_batched_lps_per_s"] / out["sequential_lps_per_s"]
    out["mpc_over_hsd_batched"] = out["mpc_batched_lps_per_s"] / out["hsd_batched_lps_per_s"]
    out["objective_max_rel_diff"] = float(np.max(np.abs(zb - zs) / (1 + np.abs(zs))))
    out["objective_max_rel_diff_to_hsd_batched"] = float(np.max(np.abs(zb - zh) / (1 + np.abs(zh))))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,64,512")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--system", default="K1")
    ap.add_argument("--worker", type=int, default=0)
    ap.add_argument("--skip-parked", type=int, choices=[0, 1], default=0, help="0 (default): parked blocks are factorised and swept like the others; 1: skipped")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_batch_bench.json"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.reps, a.system, a.skip_parked)
    res = []
    for B in (int(s) for s in a.sizes.split(",")):
        limit = LIMIT_S.get(B, 600)
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--worker", str(B), "--reps", str(a.reps),
                            "--system", a.system, "--skip-parked", str(a.skip_parked)], stdout=subprocess.PIPE, text=True)     # (the child's progress notes go straight to stderr)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"B = {B}: exit status {p.returncode}; nothing more is started on the GPU\n{p.stdout[-2000:]}", flush=True)
            break
        res.append(json.loads(line[0][len("RESULT "):]))
        print(json.dumps(res[-1]), flush=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/mpc_batch_bench.py", "results": res}, f, indent=1)
    return 0 if len(res) == len(a.sizes.split(",")) else 1


if __name__ == "__main__":
    sys.exit(main())
