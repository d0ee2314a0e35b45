"""K1 with dense columns (tlpk_options.dense_cols) against K2 and plain K1 on LPs with dense / linking columns.

One JSON line per (workload, system): ms per Newton step (1 update! + 4 solves, the first two as a pair, as bench.py counts it),
nnz(L), device bytes, host analyse time and the larger of the two augmented-system residuals of the last solve (tests/helpers.py:
kkt_residuals).  A configuration that does not fit or fails reports its status instead.  Workloads, all seeded:
  W1  Chebyshev (L-inf) regression  min t  s.t. |M beta - y| <= t, M sparse (banded): the t column touches every row;
      m = 2 q = 16 000 (plain K1 feasible: one dense 16k front) and m = 200 000 (dense_cols and K2 only);
  W2  two-stage stochastic LP shaped like config C4: 64 scenarios W_s (5000 x 10 000, 4 nonzeros per column, as
      workloads.block_angular_lp) and 200 first-stage columns touching 20 rows of every scenario; K1 + detect_blocks,
      K1 + dense_cols + detect_blocks, K2 + detect_blocks.
    python tools/dense_cols_bench.py [--steps 5] [--warmup 2] [--only W1_16k,W1_200k,W2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20261016


def chebyshev(q, p, seed=SEED, nnz_row=4):
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(q), nnz_row)
    cols = (((np.arange(q) * p) // q)[:, None] + np.arange(nnz_row)[None, :]).ravel() % p
    M = sp.csr_matrix((rng.standard_normal(q * nnz_row), (rows, cols)), shape=(q, p))
    M.sum_duplicates()
    e = sp.csc_matrix(np.ones((q, 1)))
    I = sp.identity(q, format="csc")
    Z = sp.csc_matrix((q, q))
    A = sp.vstack([sp.hstack([M, -e, I, Z]), sp.hstack([-M, -e, Z, I])], format="csc")
    A.sort_indices()
    return A


def two_stage(S=64, mk=5000, nk=10000, k=200, per=20, seed=SEED):
    import workloads
    W, _ = workloads.block_angular_lp(nblocks=S, mk=mk, nk=nk, m0=0, nnz_in=4, seed=seed)
    rng = np.random.default_rng(seed + 1)
    rows = np.concatenate([s * mk + np.sort(rng.choice(mk, size=per, replace=False)) for _ in range(k) for s in range(S)])
    cols = np.repeat(np.arange(k), S * per)
    T = sp.csc_matrix((rng.standard_normal(rows.size), (rows, cols)), shape=(S * mk, k))
    A = sp.hstack([T, W], format="csc")
    A.sort_indices()
    return A


def kkt_residual(A, th, rp, rd, xp, xd, dx, dy):
    r_p = A @ dx + rd * dy - xp
    r_d = -dx * (th + rp) + A.T @ dy - xd
    return float(max(np.abs(r_p).max(initial=0.0), np.abs(r_d).max(initial=0.0)))


def run(name, A, system, steps, warmup, torch, dev, **kw):
    import tulip_jl_amd as tk
    m, n = A.shape
    out = {"workload": name, "system": system, "options": {k_: (v if isinstance(v, (int, str)) else "list") for k_, v in kw.items()},
           "m": m, "n": n, "nnzA": int(A.nnz)}
    try:
        kkt = tk.setup(A, tk.K2() if system == "K2" else tk.K1(), tk.Backend(device=0, **kw))
    except Exception as e:                       # noqa: BLE001 -- reported, not raised: what does not fit is a result
        out.update(status=type(e).__name__, message=str(e)[:300])
        return out
    rng = np.random.default_rng(SEED)
    th = 10.0 ** rng.uniform(-3, 3, n); rp = np.full(n, 1e-4); rd = np.full(m, 1e-4)
    xp, xd, xp1, xd1 = rng.standard_normal(m), rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(n)
    T = lambda v: torch.from_numpy(v).to(dev)    # noqa: E731
    d = [T(v) for v in (th, rp, rd, xp, xd, xp1, xd1)]
    o = [torch.empty(sz, dtype=torch.float64, device=dev) for sz in (n, m, n, m, n, m, n, m)]
    P = lambda t: t.data_ptr()                   # noqa: E731

    def step():
        kkt.update_device(P(d[0]), P(d[1]), P(d[2]))
        kkt.solve2_device(P(o[0]), P(o[1]), P(d[3]), P(d[4]), P(o[2]), P(o[3]), P(d[5]), P(d[6]), sync=False)
        kkt.solve_device(P(o[4]), P(o[5]), P(d[3]), P(d[4]), sync=False)
        kkt.solve_device(P(o[6]), P(o[7]), P(d[5]), P(d[6]), sync=False)
        kkt.sync()

    try:
        for _ in range(warmup):
            step()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        ms = 1e3 * (time.perf_counter() - t0) / steps
    except Exception as e:                       # noqa: BLE001
        out.update(status=type(e).__name__, message=str(e)[:300])
        return out
    st = kkt.stats()
    dx, dy = o[4].cpu().numpy(), o[5].cpu().numpy()
    out.update(status="ok", ms_per_step=ms, nnzL=int(st["nnzL"]), device_bytes=int(st["device_bytes"]), ms_analyse=float(st["ms_analyse"]),
               n_dense_cols=int(st["n_dense_cols"]), n_blocks=int(st["n_blocks"]), max_front=int(st["max_front"]),
               max_residual=kkt_residual(A, th, rp, rd, xp, xd, dx, dy))
    kkt.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="W1_16k,W1_200k,W2")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    dev = torch.device("cuda", 0)
    torch.ones(1, device=dev)
    only = set(a.only.split(","))
    jobs = []
    if "W1_16k" in only:
        A = chebyshev(8000, 8000)
        jobs += [("W1_16k", A, "K1", {}), ("W1_16k", A, "K1", {"dense_cols": "auto"}), ("W1_16k", A, "K2", {})]
    if "W1_200k" in only:
        A = chebyshev(100000, 100000)
        jobs += [("W1_200k", A, "K1", {"dense_cols": "auto"}), ("W1_200k", A, "K2", {})]
    if "W2" in only:
        A = two_stage()
        jobs += [("W2", A, "K1", {"row_block": "auto"}), ("W2", A, "K1", {"row_block": "auto", "dense_cols": "auto"}),
                 ("W2", A, "K2", {"row_block": "auto"})]
    for name, A, system, kw in jobs:
        print(json.dumps(run(name, A, system, a.steps, a.warmup, torch, dev, **kw)), flush=True)


if __name__ == "__main__":
    main()
