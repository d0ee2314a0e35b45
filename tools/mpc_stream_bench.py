"""More LPs than slots through Mehrotra's loop: BatchedDeviceMPC.optimize_stream against successive whole batches.

Inputs: N = 4096 copies of tests/golden/stair25.mps with the seeded cost perturbations of tools/hsd_batch_bench.py (every copy has an optimum).
For B = 64 and B = 512 slots and skip_parked off and on, each in a process of its own:
  stream   the first B copies load the handle, the other N - B stream through it: optimize_stream -- a finished slot takes the next LP, which
           ENTERS through the update and the two solves of the running LPs (tlpk_mpc_batch_*_enter); records through tlpk_ipm_get_lps
  stream, per-LP records   the same with the four tlpk_ipm_get_lp reads per leaving LP that the HSD stream was measured with (one run)
  rounds   N / B successive reload(c=...) + optimize() rounds on ONE analysed handle, results read after every round: the baseline
Median of three runs each.  Per (B, skip_parked), written to profiles/mpc_stream_bench.json (also printed line by line): LPs per second, passes,
ms per pass, corrector rounds per pass, the shares of the wall time spent in refills, in tlpk_mpc_batch_enter_finish and in reading records (with
and without the gather), whether every LP ends with the status and the iteration count of the rounds, and the largest relative objective difference.
Every case runs in a child process under `timeout`; the driver stops at the first one that fails.

    python tools/mpc_stream_bench.py [--slots 64,512] [--n 4096] [--reps 3] [--system K1] [--skip-parked 0,1]
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
LIMIT_S = 540          # per child process


def worker(B, N, reps, system, skip=0):
    from hsd_batch_bench import costs
    from tulip_jl_amd.mpc_batch import BatchedDeviceMPC
    from tulip_jl_amd.problem import read_free_mps, standard_form
    d = standard_form(read_free_mps(os.path.join(ROOT, "tests", "golden", "stair25.mps")))
    assert N % B == 0 and N >= B
    cs = costs(d, N)
    lp = lambda c: (d.A, d.b, c, d.l, d.u, d.c0, d.objsense)                             # noqa: E731
    med = lambda v: float(np.median(np.asarray(v, dtype=float)))                         # noqa: E731
    out = {"B": B, "N": N, "system": system, "m": int(d.A.shape[0]), "n": int(d.A.shape[1]), "nnzA": int(d.A.nnz), "reps": reps, "skip_parked": int(skip)}
    t0 = time.perf_counter()
    opt = BatchedDeviceMPC([lp(c) for c in cs[:B]], system=system, device=0, skip_parked=bool(skip))
    out["setup_s"] = time.perf_counter() - t0

    def stream():
        opt.reload(c=np.concatenate(cs[:B]))                                             # back to the first occupants (not timed)
        t0 = time.perf_counter()
        recs = opt.optimize_stream([lp(c) for c in cs[B:]])
        return time.perf_counter() - t0, recs

    wall, passes, refills, refill_s, finish_s, record_s = [], [], [], [], [], []
    for r in range(reps):
        w, recs = stream()
        wall.append(w); passes.append(opt.passes); refills.append(opt.refills)
        refill_s.append(opt.refill_seconds); finish_s.append(opt.enter_finish_seconds); record_s.append(opt.record_seconds)
        cor_a = opt.corrector_rounds
    sa, ia = [r["status"] for r in recs], np.array([r["niter"] for r in recs])
    za = np.array([r["primal_objective"] for r in recs])
    out.update(stream_s=med(wall), stream_lps_per_s=N / med(wall), stream_passes=int(med(passes)), stream_refill_calls=int(med(refills)),
               stream_ms_per_pass=1e3 * med(wall) / med(passes), stream_corrector_rounds_per_pass=cor_a / passes[-1],
               stream_refill_share=med(refill_s) / med(wall), stream_enter_finish_share=med(finish_s) / med(wall), stream_record_share=med(record_s) / med(wall),
               stream_ms_per_refill_call=1e3 * med(refill_s) / max(1, int(med(refills))), iterations_mean=float(ia.mean()), iterations_max=int(ia.max()),
               ideal_passes=float((ia + 1).sum() / B), stream_status={s: sa.count(s) for s in set(sa)})
    # the records as the HSD stream was measured: four blocking copies per leaving LP
    opt.gather_records = False
    w, recs1 = stream()
    opt.gather_records = True
    out.update(stream_per_lp_records_s=w, stream_per_lp_records_share=opt.record_seconds / w,
               per_lp_records_same_bytes=bool(all(np.array_equal(a[k], b[k]) for a, b in zip(recs, recs1) for k in ("x", "y", "zl", "zu"))))
    # successive rounds on the analysed handle
    wall, passes_b = [], []
    for _ in range(reps):
        sb, ib, zb, np_, cor_b = [], [], [], 0, 0
        t0 = time.perf_counter()
        for r0 in range(0, N, B):
            opt.corrector_rounds = 0
            opt.reload(c=np.concatenate(cs[r0:r0 + B])).optimize()
            cor_b += opt.corrector_rounds
            for what in (0, 3, 4, 5):
                opt._vec(what)                                                           # the results of the round: x, zl, zu, y
            sb += [str(s) for s in opt.status]; ib += opt.niter.tolist(); zb += opt.primal_objective.tolist()
            np_ += int(opt.niter.max()) + 1
        wall.append(time.perf_counter() - t0)
        passes_b.append(np_)
    ib, zb = np.array(ib), np.array(zb)
    out.update(rounds_s=med(wall), rounds_lps_per_s=N / med(wall), rounds_passes=int(med(passes_b)), rounds_ms_per_pass=1e3 * med(wall) / med(passes_b),
               rounds_corrector_rounds_per_pass=cor_b / passes_b[-1])
    opt.kkt.close()
    out["speedup_stream_over_rounds"] = out["stream_lps_per_s"] / out["rounds_lps_per_s"]
    out["same_status_and_iterations_as_rounds"] = bool(sa == sb and np.array_equal(ia, ib))
    out["objective_max_rel_diff"] = float(np.max(np.abs(za - zb) / (1 + np.abs(zb))))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="64,512")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--system", default="K1")
    ap.add_argument("--worker", type=int, default=0)
    ap.add_argument("--skip-parked", default="0,1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_stream_bench.json"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.n, a.reps, a.system, int(a.skip_parked))
    res = []
    cases = [(int(s), int(k)) for s in a.slots.split(",") for k in a.skip_parked.split(",")]
    for B, skip in cases:
        p = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--worker", str(B), "--n", str(a.n),
                            "--reps", str(a.reps), "--system", a.system, "--skip-parked", str(skip)], capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"B = {B}, skip_parked = {skip}: exit status {p.returncode}; nothing more is started on the GPU\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}", flush=True)
            break
        res.append(json.loads(line[0][len("RESULT "):]))
        print(json.dumps(res[-1]), flush=True)
        keep = {}
        if os.path.exists(a.out):                                                        # (the plain batch on this commit and on its parent, recorded beside the stream)
            try:
                keep = {k: v for k, v in json.load(open(a.out)).items() if k not in ("tool", "results")}
            except ValueError:
                keep = {}
        with open(a.out, "w") as f:
            json.dump(dict({"tool": "tools/mpc_stream_bench.py", "results": res}, **keep), f, indent=1)
    return 0 if len(res) == len(cases) else 1


if __name__ == "__main__":
    sys.exit(main())
