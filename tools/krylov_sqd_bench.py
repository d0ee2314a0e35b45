"""The matrix-free K2 backend in its quasi-definite form (tlpk_options.krylov = TLPK_KRYLOV_TRICG; DESIGN.md section 1b'''''') on the matrix of ONE
config-C4 block (5000 x 10000) and of EIGHT C4 blocks with their linking rows (41000 x 80000), workloads.py, with the MINRES handle (K2) and the
conjugate-gradient handle (K1) measured in the same run beside it, none of them preconditioned.
Written to profiles/krylov_sqd_bench.json (one JSON document; also printed).  There is no pass / fail number: the file records what the path does.

  per iteration   a solve that cannot converge (atol = rtol = 1e-300) with itmax = --iters, enqueued as ONE chunk (TLPK_CG_CHUNK): device time of the
                  solve / iterations = microseconds per iteration, launches per iteration from tlpk_stats.launches_solve; the same solve with the
                  default chunking next to it
  bytes           the byte model of one iteration, N = n + m:
                      TriCG   40 nnz + 152 N + 8 m
                        k_tc_op    both copies of A (2 x 12 nnz), the two gathers (2 x 8 nnz), the pointer arrays, W, w_old, t (32 N), v for alpha (8 m)
                        k_tc_step  t (read + write), W, 1 / W, w (40 N)
                        k_tc_upd   1 / W, t, w, w_new (32 N), the two columns of G (read + write, 32 N), x (read + write, 16 N)
                      MINRES  40 nnz + 112 N                            (tools/krylov_k2_bench.py)
                      CG      40 nnz + 24 n + 104 m                     (tools/krylov_bench.py)
                  achieved bytes/s = model / time, and its fraction of the 6.29 TB/s of a streaming copy
  unit solve      theta = Rp = Rd = 1: iterations, device and wall time of a real solve of each handle

    python tools/krylov_sqd_bench.py [--iters 400] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12          # bytes/s of a device-to-device copy on one MI355X (read + write counted)


def median(v):
    return float(np.median(np.asarray(v, dtype=float)))


def handle(tk, A, method, **kw):
    return tk.setup(A, tk.K1() if method == "cg" else tk.K2(), tk.KrylovBackend(device=0, method=method, **kw))


def one(name, A, iters, reps):
    import tulip_jl_amd as tk
    m, n = A.shape
    nnz = int(A.nnz)
    rng = np.random.default_rng(5)
    xp, xd = rng.standard_normal(m), rng.standard_normal(n)
    ones_n, ones_m = np.ones(n), np.ones(m)
    dx, dy = np.zeros(n), np.zeros(m)
    out = {"workload": name, "m": m, "n": n, "nnzA": nnz}
    for method in ("tricg", "minres", "cg"):
        fixed = 5 if method == "cg" else 2              # launches of a solve outside its iterations
        model = {"tricg": 40 * nnz + 152 * (n + m) + 8 * m, "minres": 40 * nnz + 112 * (n + m), "cg": 40 * nnz + 24 * n + 104 * m}[method]
        r = {"model_bytes_per_iteration": model}
        for label, chunk in (("one_chunk", f"{iters},{iters}"), ("default_chunks", None)):
            if chunk:
                os.environ["TLPK_CG_CHUNK"] = chunk
            else:
                os.environ.pop("TLPK_CG_CHUNK", None)
            kkt = handle(tk, A, method, itmax=iters, atol=1e-300, rtol=1e-300)
            tk.update(kkt, ones_n, ones_n, ones_m)
            ms, wall = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                tk.solve(dx, dy, kkt, xp, xd)
                wall.append(1e3 * (time.perf_counter() - t0))
                ms.append(kkt.stats()["ms_last_solve"])
            st = kkt.stats()
            assert st["krylov_iters"] == iters and st["krylov_converged"] == 0, st
            us = 1e3 * median(ms) / iters
            r[label] = {"iterations": iters, "device_ms": median(ms), "wall_ms": median(wall), "us_per_iteration": us,
                        "launches_per_iteration": (st["launches_solve"] - fixed) / iters,
                        "achieved_bytes_per_s": model / (1e-6 * us), "fraction_of_copy_rate": model / (1e-6 * us) / COPY_RATE}
            kkt.close()
        os.environ.pop("TLPK_CG_CHUNK", None)
        kkt = handle(tk, A, method)
        tk.update(kkt, ones_n, ones_n, ones_m)
        tk.solve(dx, dy, kkt, xp, xd)
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            tk.solve(dx, dy, kkt, xp, xd)
            wall.append(1e3 * (time.perf_counter() - t0))
        st = kkt.stats()
        r["unit_solve"] = {"iterations": int(st["krylov_iters"]), "converged": int(st["krylov_converged"]), "device_ms": st["ms_last_solve"],
                           "wall_ms": median(wall), "launches_solve": int(st["launches_solve"]), "update_device_ms": st["ms_last_update"],
                           "device_bytes": int(st["device_bytes"])}
        kkt.close()
        out[method] = r
        print(f"{name:16s} {method:6s}: {r['one_chunk']['us_per_iteration']:7.2f} us / iteration in one chunk "
              f"({r['default_chunks']['us_per_iteration']:7.2f} chunked), {r['one_chunk']['launches_per_iteration']:.0f} launches, "
              f"{r['one_chunk']['achieved_bytes_per_s'] / 1e9:7.1f} GB/s = {100 * r['one_chunk']['fraction_of_copy_rate']:.1f} % of the copy rate; "
              f"unit solve {r['unit_solve']['iterations']} iterations, {r['unit_solve']['device_ms']:.3f} ms", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "krylov_sqd_bench.json"))
    a = ap.parse_args()
    import tulip_jl_amd as tk
    if tk._lib.lib().tlpk_device_count() < 1:
        raise SystemExit("needs a GPU")
    from workloads import block_angular_lp
    res = []
    for name, (A, _) in (("c4_one_block", block_angular_lp(nblocks=1, m0=0)), ("c4_eight_blocks", block_angular_lp(nblocks=8))):
        r = one(name, A, a.iters, a.reps)
        print(json.dumps(r), flush=True)
        res.append(r)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/krylov_sqd_bench.py", "copy_rate_bytes_per_s": COPY_RATE, "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
