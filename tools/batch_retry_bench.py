"""Retry of the failed LPs alone against whole-batch retries: the batched HSD loop under retry="all" and retry="failed", side by side.

Inputs: copies of tests/golden/bump.mps (every copy meets non-positive pivots and bumps its regularisations many times) and of tests/golden/stair25.mps
(no copy ever bumps: the two settings must cost the same) under the seeded cost perturbations of tools/hsd_batch_bench.py, iteration limit 100, K1.
For B = 8, 64 and 512, each (LP, B) in a child process of its own under a time limit, both settings in ONE process (a handle per setting, the settings
interleaved run by run, one warm-up run each), median of `reps` timed runs.  Reported per setting: update calls per pass, LP-factorisations per pass (the
LPs the update calls were asked to factorise), ms per pass, LPs per second (a pass = one trip round the loop); and the largest relative difference of the
objectives between the two settings.  Written to profiles/batch_retry_bench.json (entries of the file that this tool does not write are kept) and printed
line by line.

    python tools/batch_retry_bench.py [--sizes 8,64,512] [--lps bump,stair25] [--reps 3] [--system K1] [--out FILE]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = {8: 120, 64: 180, 512: 420}


def med(v):
    return float(np.median(np.asarray(v, dtype=float)))


def worker(name, B, reps, system):
    from hsd_batch_bench import costs
    from tulip_jl_amd.hsd_batch import BatchedDeviceHSD
    from tulip_jl_amd.hsd_device import Options
    from tulip_jl_amd.problem import read_free_mps, standard_form

    class Hundred(Options):
        IterationsLimit = 100

    d = standard_form(read_free_mps(os.path.join(ROOT, "tests", "golden", name + ".mps")))
    lps = [(d.A, d.b, c, d.l, d.u, d.c0, d.objsense) for c in costs(d, B)]
    opts = {retry: BatchedDeviceHSD(lps, system=system, device=0, options=Hundred(), retry=retry) for retry in ("all", "failed")}
    wall, end = {"all": [], "failed": []}, {}
    for r in range(reps + 1):                                                            # (run 0 of each setting is the warm-up)
        for retry, opt in opts.items():
            t0 = time.perf_counter()
            opt.optimize()
            if r:
                wall[retry].append(time.perf_counter() - t0)
            end[retry] = dict(status=[str(s) for s in opt.status], niter=opt.niter.copy(), z=opt.primal_objective.copy(), retry=opt.retry,
                              calls=int(opt.timers["n_update_calls"]), lp_factor=int(opt.timers["n_lp_factor"]), n_bump=int(opt.timers["n_bump"].sum()),
                              multi=sum(1 for nb in opt.bump_log if (nb > 0).sum() >= 2), bump_passes=len(opt.bump_log))
    a, f = end["all"], end["failed"]
    passes = int(a["niter"].max()) + 1
    out = {"lp": name, "B": B, "system": system, "reps": reps, "m": int(d.A.shape[0]), "n": int(d.A.shape[1]), "passes": passes,
           "iterations_mean": float(a["niter"].mean()), "n_bump": a["n_bump"], "passes_with_a_bump": a["bump_passes"], "passes_with_two_or_more_failing_lps": a["multi"],
           "same_status_and_iterations": bool(a["status"] == f["status"] and np.array_equal(a["niter"], f["niter"])),
           "objective_max_rel_diff": float(np.max(np.abs(a["z"] - f["z"]) / (1 + np.abs(a["z"])))),
           "status": {s: a["status"].count(s) for s in set(a["status"])}}
    for retry in ("all", "failed"):
        e, s = end[retry], med(wall[retry])
        out[retry] = {"retry_in_force": e["retry"], "s": s, "lps_per_s": B / s, "ms_per_pass": 1e3 * s / passes, "update_calls": e["calls"],
                      "update_calls_per_pass": e["calls"] / passes, "lp_factorisations_per_pass": e["lp_factor"] / passes}
    out["speedup"] = out["failed"]["lps_per_s"] / out["all"]["lps_per_s"]
    for opt in opts.values():
        opt.kkt.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8,64,512")
    ap.add_argument("--lps", default="bump,stair25")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--system", default="K1")
    ap.add_argument("--worker", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_retry_bench.json"))
    a = ap.parse_args()
    if a.worker:
        name, B = a.worker.split(":")
        return worker(name, int(B), a.reps, a.system)
    keep = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            keep = {k: v for k, v in json.load(f).items() if k not in ("tool", "results")}
    res, want = [], 0
    for name in a.lps.split(","):
        for B in (int(s) for s in a.sizes.split(",")):
            want += 1
            p = subprocess.run(["timeout", "-k", "10", str(LIMIT_S.get(B, 420)), sys.executable, os.path.abspath(__file__), "--worker", f"{name}:{B}",
                                "--reps", str(a.reps), "--system", a.system], capture_output=True, text=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(f"{name}, B = {B}: exit status {p.returncode}; nothing more is started on the GPU\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}", flush=True)
                return 1
            res.append(json.loads(line[0][len("RESULT "):]))
            print(json.dumps(res[-1]), flush=True)
            with open(a.out, "w") as f:
                json.dump(dict({"tool": "tools/batch_retry_bench.py", "results": res}, **keep), f, indent=1)
    return 0 if len(res) == want else 1


if __name__ == "__main__":
    sys.exit(main())
