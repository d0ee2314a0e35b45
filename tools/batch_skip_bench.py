"""Parked blocks skipped or not: the batched loops under both settings of tlpk_ipm_batch_skip, side by side.

Inputs: copies of tests/golden/stair25.mps with the seeded cost perturbations of tools/hsd_batch_bench.py.  For B = 64 and B = 512, each leg in a
child process of its own, both settings on ONE handle (BatchedDeviceHSD.set_skip_parked between runs), the settings interleaved run by run, one
warm-up run per setting, median of `reps` timed runs:
  hsd     BatchedDeviceHSD.optimize() of B LPs
  mpc     BatchedDeviceMPC.optimize() of B LPs
  stream  N = 4096 LPs through B slots (optimize_stream) and the same LPs as N / B successive reload + optimize rounds, as tools/hsd_stream_bench.py
          runs them; the ratio stream / rounds per setting
skip_parked = 0 is the behaviour before the switch existed (every block factorised and swept in every update and solve) and the baseline.
Reported per setting: LPs per second, ms per pass (a pass = one trip round the loop: an iteration of the batch's slowest LP, plus the final test),
and that both settings end every LP with the same status, iteration count and objective bits.
Written to profiles/batch_skip_bench.json and printed line by line.

    python tools/batch_skip_bench.py [--sizes 64,512] [--legs hsd,mpc,stream] [--n 4096] [--reps 3] [--system K1]
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
LIMIT_S = 420


def med(v):
    return float(np.median(np.asarray(v, dtype=float)))


def batch_leg(leg, B, reps, system, d, cs):
    from tulip_jl_amd.hsd_batch import BatchedDeviceHSD
    from tulip_jl_amd.mpc_batch import BatchedDeviceMPC
    cls = BatchedDeviceMPC if leg == "mpc" else BatchedDeviceHSD
    opt = cls([(d.A, d.b, c, d.l, d.u, d.c0, d.objsense) for c in cs[:B]], system=system, device=0, skip_parked=False)
    wall, end = {0: [], 1: []}, {}
    for r in range(reps + 1):                                                            # (run 0 of each setting is the warm-up)
        for sk in (0, 1):
            opt.set_skip_parked(sk)
            t0 = time.perf_counter()
            opt.optimize()
            if r:
                wall[sk].append(time.perf_counter() - t0)
            end[sk] = ([str(s) for s in opt.status], opt.niter.copy(), opt.primal_objective.copy())
    passes = int(end[0][1].max()) + 1
    out = {"iterations_mean": float(end[0][1].mean()), "iterations_max": int(end[0][1].max()), "passes": passes,
           "same_results": bool(end[0][0] == end[1][0] and np.array_equal(end[0][1], end[1][1]) and end[0][2].tobytes() == end[1][2].tobytes())}
    for sk in (0, 1):
        out[f"skip{sk}"] = {"s": med(wall[sk]), "lps_per_s": B / med(wall[sk]), "ms_per_pass": 1e3 * med(wall[sk]) / passes}
    out["speedup"] = out["skip1"]["lps_per_s"] / out["skip0"]["lps_per_s"]
    opt.kkt.close()
    return out


def stream_leg(B, N, reps, system, d, cs):
    from tulip_jl_amd.hsd_batch import BatchedDeviceHSD
    lp = lambda c: (d.A, d.b, c, d.l, d.u, d.c0, d.objsense)                             # noqa: E731
    opt = BatchedDeviceHSD([lp(c) for c in cs[:B]], system=system, device=0, skip_parked=False)
    st, ro, info, end = {0: [], 1: []}, {0: [], 1: []}, {}, {}
    for r in range(reps):
        for sk in (0, 1):
            opt.set_skip_parked(sk)
            opt.refill(range(B), [lp(c) for c in cs[:B]])                                # back to the first occupants (not timed)
            t0 = time.perf_counter()
            recs = opt.optimize_stream([lp(c) for c in cs[B:]])
            st[sk].append(time.perf_counter() - t0)
            info[sk] = {"stream_passes": int(opt.passes), "stream_corrector_rounds_per_pass": opt.corrector_rounds / max(opt.passes, 1)}
            end[sk] = ([x["status"] for x in recs], [x["niter"] for x in recs], [x["primal_objective"] for x in recs])
            passes, cor = 0, 0
            t0 = time.perf_counter()
            for r0 in range(0, N, B):
                opt.corrector_rounds = 0
                opt.reload(c=np.concatenate(cs[r0:r0 + B])).optimize()
                cor += opt.corrector_rounds
                for what in (0, 3, 4, 5):
                    opt._vec(what)                                                       # the results of the round: x, zl, zu, y
                passes += int(opt.niter.max()) + 1
            ro[sk].append(time.perf_counter() - t0)
            info[sk].update(rounds_passes=passes, rounds_corrector_rounds_per_pass=cor / max(passes, 1))
    out = {"N": N, "same_results": bool(end[0] == end[1])}
    for sk in (0, 1):
        s, q = med(st[sk]), med(ro[sk])
        out[f"skip{sk}"] = dict(info[sk], stream_s=s, stream_lps_per_s=N / s, stream_ms_per_pass=1e3 * s / info[sk]["stream_passes"], rounds_s=q,
                                rounds_lps_per_s=N / q, rounds_ms_per_pass=1e3 * q / info[sk]["rounds_passes"], stream_over_rounds=q / s)
    out["speedup_stream"] = out["skip1"]["stream_lps_per_s"] / out["skip0"]["stream_lps_per_s"]
    out["speedup_rounds"] = out["skip1"]["rounds_lps_per_s"] / out["skip0"]["rounds_lps_per_s"]
    opt.kkt.close()
    return out


def worker(leg, B, N, reps, system):
    from hsd_batch_bench import costs
    from tulip_jl_amd.problem import read_free_mps, standard_form
    d = standard_form(read_free_mps(os.path.join(ROOT, "tests", "golden", "stair25.mps")))
    cs = costs(d, N if leg == "stream" else B)
    out = {"leg": leg, "B": B, "system": system, "reps": reps}
    out.update(stream_leg(B, N, reps, system, d, cs) if leg == "stream" else batch_leg(leg, B, reps, system, d, cs))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,512")
    ap.add_argument("--legs", default="hsd,mpc,stream")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--system", default="K1")
    ap.add_argument("--worker", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_skip_bench.json"))
    a = ap.parse_args()
    if a.worker:
        leg, B = a.worker.split(":")
        return worker(leg, int(B), a.n, a.reps, a.system)
    res, want = [], 0
    for leg in a.legs.split(","):
        for B in (int(s) for s in a.sizes.split(",")):
            want += 1
            p = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--worker", f"{leg}:{B}", "--n", str(a.n),
                                "--reps", str(a.reps), "--system", a.system], capture_output=True, text=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(f"{leg}, B = {B}: exit status {p.returncode}; nothing more is started on the GPU\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}", flush=True)
                return 1
            res.append(json.loads(line[0][len("RESULT "):]))
            print(json.dumps(res[-1]), flush=True)
            with open(a.out, "w") as f:
                json.dump({"tool": "tools/batch_skip_bench.py", "results": res}, f, indent=1)
    return 0 if len(res) == want else 1


if __name__ == "__main__":
    sys.exit(main())
