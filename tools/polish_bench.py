"""Refinement on demand (tlpk_polish_device / tlpk_polish2_device / tlpk_ipm_set_polish; DESIGN.md section 1c') against what existed before it, on the matrix
of ONE config-C4 block (5000 x 10000) and of EIGHT C4 blocks with their linking rows (41000 x 80000), workloads.py.  Written to profiles/polish_bench.json
(one JSON document; also printed).  The two legs of every comparison ALTERNATE in one process, --reps times after a warm-up of each; wall time of the
calls + tlpk_sync around device buffers; median and spread (min, max) of each leg.

  (a) K1   tlpk_solve2_device + tlpk_polish2_device(steps = 1) on a refine_steps = 0 handle against two tlpk_solve_device on a refine_steps = 1 handle (what
           tlpk_solve2_device falls back to there): the same four vectors, compared for equality
  (b) K2   tlpk_polish2_device(1) against two tlpk_polish_device(1), after the same tlpk_solve2_device: compared for equality
  (c)      DeviceHSD on the one-block LP, --hsd-iters interior-point iterations: time per iteration with polish = 1 on a refine = 0 handle against a
           refine = 1 handle (K1); status, iteration count and objective compared for equality

    python tools/polish_bench.py [--reps 9]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from krylov_pair_bench import DevBuf, spread  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def alternate(legs, reps):
    """legs: name -> callable.  Two warm-up calls of each, then `reps` rounds in turn; name -> wall times (ms)."""
    for fn in legs.values():
        fn(); fn()
    out = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            out[k].append(timed(fn))
    return out


def one(workload, A, row_block, reps):
    import tulip_jl_amd as tk
    m, n = A.shape
    rng = np.random.default_rng(5)
    th = 10.0 ** rng.uniform(-3, 3, n); rp = np.full(n, 1e-4); rd = np.full(m, 1e-4)
    rhs = [(rng.standard_normal(m), rng.standard_normal(n)) for _ in range(2)]
    kw = {} if row_block is None else {"row_block": row_block}
    res = {"workload": workload, "m": m, "n": n, "nnzA": int(A.nnz), "reps": reps}

    def bufs():
        return [DevBuf(v) for r in rhs for v in r], [DevBuf(n), DevBuf(m), DevBuf(n), DevBuf(m)]

    # (a) K1
    plain = tk.setup(A, tk.K1(), tk.Backend(device=0, **kw)); tk.update(plain, th, rp, rd)
    ref = tk.setup(A, tk.K1(), tk.Backend(device=0, refine=1, **kw)); tk.update(ref, th, rp, rd)
    ip, op = bufs(); ir, orf = bufs()

    def pair_polish():
        plain.solve2_device(op[0].ptr, op[1].ptr, ip[0].ptr, ip[1].ptr, op[2].ptr, op[3].ptr, ip[2].ptr, ip[3].ptr, sync=False)
        plain.polish2_device(op[0].ptr, op[1].ptr, ip[0].ptr, ip[1].ptr, op[2].ptr, op[3].ptr, ip[2].ptr, ip[3].ptr, steps=1)

    def two_refined():
        ref.solve_device(orf[0].ptr, orf[1].ptr, ir[0].ptr, ir[1].ptr, sync=False)
        ref.solve_device(orf[2].ptr, orf[3].ptr, ir[2].ptr, ir[3].ptr)

    def pair_plain():
        plain.solve2_device(op[0].ptr, op[1].ptr, ip[0].ptr, ip[1].ptr, op[2].ptr, op[3].ptr, ip[2].ptr, ip[3].ptr)

    t = alternate({"solve2_polish2": pair_polish, "two_refined_solves": two_refined}, reps)
    equal = all(a.get().tobytes() == b.get().tobytes() for a, b in zip(op, orf))
    u = alternate({"solve2_unrefined": pair_plain}, reps)
    a_, b_ = spread(t["solve2_polish2"]), spread(t["two_refined_solves"])
    res["a_k1"] = {"solve2_polish2_ms": a_, "two_refined_solves_ms": b_, "ratio": a_["median"] / b_["median"], "outputs_equal": bool(equal),
                   "solve2_unrefined_ms": spread(u["solve2_unrefined"]), "report": plain.polish_report(),
                   "two_refined_spread_max_over_min": b_["max"] / b_["min"]}
    plain.close(); ref.close()
    print(json.dumps({workload: {"a_k1": res["a_k1"]}}), flush=True)

    # (b) K2
    k2 = tk.setup(A, tk.K2(), tk.Backend(device=0, **kw)); tk.update(k2, th, rp, rd)
    i2, base = bufs()
    k2.solve2_device(base[0].ptr, base[1].ptr, i2[0].ptr, i2[1].ptr, base[2].ptr, base[3].ptr, i2[2].ptr, i2[3].ptr)
    start = [b.get() for b in base]
    o_pair, o_two = [DevBuf(v) for v in start], [DevBuf(v) for v in start]
    hip = DevBuf._hip

    def reset(dst):
        for d, s in zip(dst, base):
            assert hip.hipMemcpy(d.ptr, s.ptr, 8 * d.n, 3) == 0             # device to device: both legs start from the unrefined pair

    def polish2():
        k2.polish2_device(o_pair[0].ptr, o_pair[1].ptr, i2[0].ptr, i2[1].ptr, o_pair[2].ptr, o_pair[3].ptr, i2[2].ptr, i2[3].ptr, steps=1)

    def two_polish():
        k2.polish_device(o_two[0].ptr, o_two[1].ptr, i2[0].ptr, i2[1].ptr, steps=1, sync=False)
        k2.polish_device(o_two[2].ptr, o_two[3].ptr, i2[2].ptr, i2[3].ptr, steps=1)

    legs = {"polish2": (polish2, o_pair), "two_polish": (two_polish, o_two)}
    report = None
    for fn, o in legs.values():
        reset(o); fn()
        report = report or k2.polish_report()                                # (of the pair: the first leg)
    equal = all(a.get().tobytes() == b.get().tobytes() for a, b in zip(o_pair, o_two))
    t = {k: [] for k in legs}
    for _ in range(reps):
        for k, (fn, o) in legs.items():
            reset(o)
            t[k].append(timed(fn))
    a_, b_ = spread(t["polish2"]), spread(t["two_polish"])
    res["b_k2"] = {"polish2_ms": a_, "two_polish_ms": b_, "ratio": a_["median"] / b_["median"], "outputs_equal": bool(equal), "report_of_the_pair": report,
                   "polish_bytes": int(k2.symbolic("polish_bytes")[0]), "device_bytes": int(k2.stats()["device_bytes"]),
                   "two_polish_spread_max_over_min": b_["max"] / b_["min"]}
    k2.close()
    print(json.dumps({workload: {"b_k2": res["b_k2"]}}), flush=True)
    return res


def hsd(A, hsd_iters, reps):
    from tulip_jl_amd.hsd_device import DeviceHSD, Options
    m, n = A.shape
    rng = np.random.default_rng(20260927)
    xs = rng.uniform(0.0, 1.0, n) * (rng.random(n) < 0.6)
    b = A @ xs
    ys = rng.standard_normal(m)
    c = A.T @ ys + rng.uniform(0.0, 1.0, n) * (xs == 0.0)
    l = np.zeros(n); u = np.full(n, np.inf)

    class Few(Options):
        IterationsLimit = hsd_iters

    opts = {"polish": DeviceHSD(A, b, c, l, u, options=Few(), device=0, polish=1), "refine": DeviceHSD(A, b, c, l, u, options=Few(), device=0, refine=1)}
    runs = {k: [] for k in opts}
    for rep in range(reps + 1):              # (the first round of both legs is the warm-up)
        for leg, opt in opts.items():
            t0 = time.perf_counter()
            opt.optimize()
            sec = time.perf_counter() - t0
            if rep:
                runs[leg].append({"status": opt.status, "iterations": int(opt.niter), "objective": float(opt.primal_objective).hex(),
                                  "ms_per_iteration": 1e3 * sec / max(opt.niter, 1)})
    for opt in opts.values():
        opt.kkt.close()
    p, r = runs["polish"], runs["refine"]
    same = all((a["status"], a["iterations"], a["objective"]) == (b_["status"], b_["iterations"], b_["objective"]) for a, b_ in zip(p, r))
    ps, rs = spread([x["ms_per_iteration"] for x in p]), spread([x["ms_per_iteration"] for x in r])
    return {"workload": "c4_one_block LP, DeviceHSD, K1", "hsd_iterations_limit": hsd_iters, "status": p[0]["status"], "iterations": p[0]["iterations"],
            "status_iterations_objective_equal": bool(same), "polish_ms_per_iteration": ps, "refine_handle_ms_per_iteration": rs,
            "ratio": ps["median"] / rs["median"], "refine_handle_spread_max_over_min": rs["max"] / rs["min"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--hsd-iters", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polish_bench.json"))
    a = ap.parse_args()
    import tulip_jl_amd as tk
    if tk._lib.lib().tlpk_device_count() < 1:
        raise SystemExit("needs a GPU")
    from workloads import block_angular_lp
    doc = {"tool": "tools/polish_bench.py", "results": []}

    def save():
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)

    A1 = None
    for name, kw in (("c4_one_block", dict(nblocks=1, m0=0)), ("c4_eight_blocks", dict(nblocks=8))):
        A, rb = block_angular_lp(**kw)
        A1 = A if A1 is None else A1
        doc["results"].append(one(name, A, rb if kw["nblocks"] > 1 else None, a.reps))
        save()
    doc["c_device_hsd"] = hsd(A1, a.hsd_iters, max(3, a.reps // 2))
    print(json.dumps(doc["c_device_hsd"]), flush=True)
    save()


if __name__ == "__main__":
    main()
