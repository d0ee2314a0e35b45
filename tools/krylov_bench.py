"""The matrix-free K1 backend (tlpk_options.krylov; DESIGN.md section 1b'''') on the matrix of ONE config-C4 block (5000 x 10000) and of EIGHT
C4 blocks with their linking rows (41000 x 80000), workloads.py.  Written to profiles/krylov_bench.json (one JSON document; also printed):

  per iteration   a solve that cannot converge (atol = rtol = 1e-300) with itmax = --iters, enqueued as ONE chunk (TLPK_CG_CHUNK): device time of the
                  solve / iterations = microseconds per iteration, launches per iteration from tlpk_stats.launches_solve; the same solve with the
                  default chunking (4, 8, 16, 32, 32, ...: a host round trip between chunks) next to it
  bytes           the byte model of one iteration
                      40 nnz + 24 n + 104 m   (+ 16 m with Jacobi)
                  = two passes over A's values and indices (2 x 12 nnz), the two gathers (p by the column pass, t by the row pass: 2 x 8 nnz), the
                  pointer arrays (8 n + 8 m), D and t (16 n), Rd, p, q in the row pass (24 m), x, r (read + write), p, q in the step (48 m), r and p
                  (read + write) in the direction update (24 m); achieved bytes/s = model / time, and its fraction of the 6.29 TB/s of a streaming copy
  chunk sweep     wall and device time, launches of the "unit" solve and of the --iters solve for several (first chunk, cap) pairs (TLPK_CG_CHUNK);
                  (1, 1) is a host round trip per iteration
  against direct  "unit" regime (theta = Rp = Rd = 1): update! and solve! of a Krylov handle (none / Jacobi; iterations) and of the direct handle

    python tools/krylov_bench.py [--iters 400] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNKS = ((1, 1), (4, 32), (8, 64), (16, 64), (16, 128), (32, 128), (32, 256), (64, 256))   # (first chunk, cap) of the chunk sweep
COPY_RATE = 6.29e12          # bytes/s of a device-to-device copy on one MI355X (read + write counted)


def median(v):
    return float(np.median(np.asarray(v, dtype=float)))


def timed(kkt, fn, reps):
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append(1e3 * (time.perf_counter() - t0))
    return median(wall)


def one(name, A, row_block, iters, reps):
    import tulip_jl_amd as tk
    m, n = A.shape
    nnz = int(A.nnz)
    rng = np.random.default_rng(5)
    xp, xd = rng.standard_normal(m), rng.standard_normal(n)
    ones_n, ones_m = np.ones(n), np.ones(m)
    dx, dy = np.zeros(n), np.zeros(m)
    out = {"workload": name, "m": m, "n": n, "nnzA": nnz}
    for pre in (None, "jacobi"):
        key = pre or "none"
        model = 40 * nnz + 24 * n + 104 * m + (16 * m if pre else 0)
        r = {"model_bytes_per_iteration": model}
        for label, chunk in (("one_chunk", f"{iters},{iters}"), ("default_chunks", None)):
            if chunk:
                os.environ["TLPK_CG_CHUNK"] = chunk
            else:
                os.environ.pop("TLPK_CG_CHUNK", None)
            kkt = tk.setup(A, tk.K1(), tk.KrylovBackend(device=0, precond=pre, itmax=iters, atol=1e-300, rtol=1e-300))
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
                        "launches_per_iteration": (st["launches_solve"] - 5) / iters,
                        "achieved_bytes_per_s": model / (1e-6 * us), "fraction_of_copy_rate": model / (1e-6 * us) / COPY_RATE}
            kkt.close()
        os.environ.pop("TLPK_CG_CHUNK", None)
        # a real solve, unit regime
        t0 = time.perf_counter()
        kkt = tk.setup(A, tk.K1(), tk.KrylovBackend(device=0, precond=pre))
        r["setup_s"] = time.perf_counter() - t0
        r["update_wall_ms"] = timed(kkt, lambda: tk.update(kkt, ones_n, ones_n, ones_m), reps)
        r["update_device_ms"] = kkt.stats()["ms_last_update"]
        r["solve_wall_ms"] = timed(kkt, lambda: tk.solve(dx, dy, kkt, xp, xd), reps)
        st = kkt.stats()
        r.update(solve_device_ms=st["ms_last_solve"], iterations=int(st["krylov_iters"]), converged=int(st["krylov_converged"]),
                 launches_solve=int(st["launches_solve"]), device_bytes=int(st["device_bytes"]))
        dy_k = dy.copy()
        kkt.close()
        # the chunking: first chunk and cap (TLPK_CG_CHUNK is read at create), on the real solve above and on the --iters solve that cannot converge
        r["chunk_sweep"] = []
        for first, cap in CHUNKS:
            os.environ["TLPK_CG_CHUNK"] = f"{first},{cap}"
            row = {"first": first, "max": cap}
            for label, kw in (("unit", {}), ("long", {"itmax": iters, "atol": 1e-300, "rtol": 1e-300})):
                kkt = tk.setup(A, tk.K1(), tk.KrylovBackend(device=0, precond=pre, **kw))
                tk.update(kkt, ones_n, ones_n, ones_m)
                tk.solve(dx, dy, kkt, xp, xd)
                row[label + "_wall_ms"] = timed(kkt, lambda: tk.solve(dx, dy, kkt, xp, xd), reps)
                st = kkt.stats()
                row.update({label + "_device_ms": st["ms_last_solve"], label + "_iterations": int(st["krylov_iters"]),
                            label + "_launches": int(st["launches_solve"])})
                kkt.close()
            r["chunk_sweep"].append(row)
        os.environ.pop("TLPK_CG_CHUNK", None)
        out[key] = r
    t0 = time.perf_counter()
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=0, row_block=row_block))
    d = {"setup_s": time.perf_counter() - t0}
    d["update_wall_ms"] = timed(kkt, lambda: tk.update(kkt, ones_n, ones_n, ones_m), reps)
    d["update_device_ms"] = kkt.stats()["ms_last_update"]
    d["solve_wall_ms"] = timed(kkt, lambda: tk.solve(dx, dy, kkt, xp, xd), reps)
    st = kkt.stats()
    d.update(solve_device_ms=st["ms_last_solve"], device_bytes=int(st["device_bytes"]), nnzL=int(st["nnzL"]))
    d["krylov_vs_direct_rel_diff_dy"] = float(np.linalg.norm(dy_k - dy) / np.linalg.norm(dy))
    kkt.close()
    out["direct"] = d
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "krylov_bench.json"))
    a = ap.parse_args()
    import tulip_jl_amd as tk
    if tk._lib.lib().tlpk_device_count() < 1:
        raise SystemExit("needs a GPU")
    from workloads import block_angular_lp
    res = []
    for name, (A, rb) in (("c4_one_block", block_angular_lp(nblocks=1, m0=0)), ("c4_eight_blocks", block_angular_lp(nblocks=8))):
        r = one(name, A, rb if name != "c4_one_block" else None, a.iters, a.reps)
        print(json.dumps(r), flush=True)
        res.append(r)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/krylov_bench.py", "copy_rate_bytes_per_s": COPY_RATE, "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
