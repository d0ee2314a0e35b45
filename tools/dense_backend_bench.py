"""Dense-matrix K1 backend (tk.DenseBackend / tlpk_create_dense) on dense A = randn(m, n), "mid" interior-point data.

One JSON line per shape (stdout, and appended to --out): ms per Newton step (1 update! + 4 solves, the first two as a pair, as
bench.py counts a step), ms per update! and per solve!, the per-class kernel times of one profiled update! + solve!, device bytes, and
  syrk    flops_syrk = n m (m + 1) over the time of the ASSEMBLE class (D + k_dense_syrk [+ its split-K reduction]), as a fraction of
          the fp64 matrix peak bench.py uses for roofline.frac; next to it k_update's roofline.frac of a `bench.py --full` line of the
          same session, if --bench-json names the file that holds it
  gemv    8 m n bytes of A per product over the time of the SPMV class of one solve (two products + two vector kernels), in TB/s
  torch   the three-line version on the same GPU: torch.linalg.cholesky((A * D) @ A.T + diag(rd)), torch.cholesky_solve
  numpy   the same on the host's CPUs (LAPACK through numpy / scipy)
and the larger augmented-system residual of the library's last solve (tests/helpers.py: kkt_residuals).
    python tools/dense_backend_bench.py [--shapes 2048x4096,...] [--steps 5] [--warmup 2] [--repeats 3] [--bench-json FILE] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20261016
FP64_MFMA_PEAK_TFLOPS = 78.6        # the peak of bench.py's roofline.frac
SHAPES = "2048x4096,4096x8192,8192x16384,16384x32768"


def windows(fn, sync, steps, warmup, repeats):
    """ms per call of fn: `repeats` timed windows of `steps` calls, each ended by a synchronise; (median, min, max) of the window means."""
    for _ in range(warmup):
        fn()
    sync()
    res = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        sync()
        res.append(1e3 * (time.perf_counter() - t0) / steps)
    return statistics.median(res), min(res), max(res)


def run(m, n, a, torch, dev, bench_ref):
    import tulip_jl_amd as tk
    rng = np.random.default_rng(SEED + m)
    A = np.empty((m, n), order="F")
    for j in range(0, n, 1024):
        A[:, j: j + 1024] = rng.standard_normal((m, min(1024, n - j)))
    th = 10.0 ** rng.uniform(-3, 3, n); rp = np.full(n, 1e-4); rd = np.full(m, 1e-4)
    xp, xd, xp1, xd1 = rng.standard_normal(m), rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(n)
    out = {"m": m, "n": n, "regime": "mid", "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
    t0 = time.perf_counter()
    kkt = tk.setup(A, tk.K1(), tk.DenseBackend(device=0))
    out["ms_setup"] = 1e3 * (time.perf_counter() - t0)
    T = lambda v: torch.from_numpy(v).to(dev)    # noqa: E731
    d = [T(v) for v in (th, rp, rd, xp, xd, xp1, xd1)]
    o = [torch.empty(sz, dtype=torch.float64, device=dev) for sz in (n, m, n, m, n, m, n, m)]
    P = lambda t: t.data_ptr()                   # noqa: E731

    def update():
        kkt.update_device(P(d[0]), P(d[1]), P(d[2]))

    def solve():
        kkt.solve_device(P(o[4]), P(o[5]), P(d[3]), P(d[4]), sync=False)

    def step():
        update()
        kkt.solve2_device(P(o[0]), P(o[1]), P(d[3]), P(d[4]), P(o[2]), P(o[3]), P(d[5]), P(d[6]), sync=False)
        solve()
        kkt.solve_device(P(o[6]), P(o[7]), P(d[5]), P(d[6]), sync=False)
        kkt.sync()

    out["ms_per_step"], out["ms_per_step_min"], out["ms_per_step_max"] = windows(step, kkt.sync, a.steps, a.warmup, a.repeats)
    out["ms_update"], out["ms_update_min"], out["ms_update_max"] = windows(update, kkt.sync, a.steps, 1, a.repeats)
    out["ms_solve"], out["ms_solve_min"], out["ms_solve_max"] = windows(solve, kkt.sync, 4 * a.steps, 2, a.repeats)
    st = kkt.stats()
    out.update(device_bytes=int(st["device_bytes"]), flops_syrk=float(st["flops_syrk"]), flops_chol=float(st["flops_chol"]), ms_analyse=float(st["ms_analyse"]),
               chain_launches=int(st["chain_launches"]))
    # per-class kernel times: one update! + one solve! with per-launch events
    kkt.set_profile(True)
    update(); solve(); kkt.sync()
    kt = kkt.kernel_times()
    kkt.set_profile(False)
    out["kernel_times"] = {k: {"ms": v["ms"], "launches": v["launches"]} for k, v in kt.items() if v["launches"]}
    asm = kt["assemble"]["ms"]
    out["syrk"] = {"ms": asm, "tflops": st["flops_syrk"] / (asm * 1e-3) / 1e12 if asm > 0 else None,
                   "frac": st["flops_syrk"] / (asm * 1e-3) / 1e12 / FP64_MFMA_PEAK_TFLOPS if asm > 0 else None, "peak_tflops": FP64_MFMA_PEAK_TFLOPS,
                   "k_update_frac_same_session": bench_ref.get("roofline_frac")}
    spmv = kt["spmv"]["ms"]
    out["gemv"] = {"ms_two_products": spmv, "tb_per_s": 2 * 8.0 * m * n / (spmv * 1e-3) / 1e12 if spmv > 0 else None,
                   "sweep_gb_per_s_same_session": bench_ref.get("solve_gbs")}
    dx, dy = o[4].cpu().numpy(), o[5].cpu().numpy()
    r_p = A @ dx + rd * dy - xp
    r_d = -dx * (th + rp) + A.T @ dy - xd
    out["max_residual"] = float(max(np.abs(r_p).max(), np.abs(r_d).max()))
    kkt.close()

    # (a) the three-line torch version on the same GPU
    try:
        At = T(np.ascontiguousarray(A.T)).T               # column-major on the device, like ours
        D = 1.0 / (d[0] + d[1])
        hold = {}

        def t_update():
            hold["L"] = torch.linalg.cholesky((At * D) @ At.T + torch.diag(d[2]))

        def t_solve():
            y = torch.cholesky_solve((d[3] + At @ (D * d[4]))[:, None], hold["L"])[:, 0]
            hold["dy"] = y; hold["dx"] = D * (At.T @ y - d[4])

        sync = torch.cuda.synchronize
        tu = windows(t_update, sync, a.steps, 1, a.repeats)
        ts = windows(t_solve, sync, 4 * a.steps, 2, a.repeats)
        err = float((hold["dy"] - o[5]).abs().max() / max(1.0, float(o[5].abs().max())))
        out["torch"] = {"ms_update": tu[0], "ms_update_min": tu[1], "ms_update_max": tu[2], "ms_solve": ts[0], "dy_rel_diff_to_library": err}
        del At, hold
        torch.cuda.empty_cache()
    except Exception as e:                               # noqa: BLE001 -- reported, not raised: what this torch build cannot do is a result
        out["torch"] = {"status": type(e).__name__, "message": str(e)[:300]}

    # (b) numpy / LAPACK on the host's CPUs
    if m <= a.numpy_max_m:
        import scipy.linalg as sla
        Dn = 1.0 / (th + rp)
        t0 = time.perf_counter()
        K = (A * Dn) @ A.T + np.diag(rd)
        Ln = np.linalg.cholesky(K)
        t1 = time.perf_counter()
        y = sla.solve_triangular(Ln, xp + A @ (Dn * xd), lower=True)
        y = sla.solve_triangular(Ln.T, y, lower=False)
        xn = Dn * (A.T @ y - xd)
        t2 = time.perf_counter()
        out["numpy"] = {"ms_update": 1e3 * (t1 - t0), "ms_solve": 1e3 * (t2 - t1), "threads": int(os.environ.get("OMP_NUM_THREADS", "0") or 0),
                        "dy_rel_diff_to_library": float(np.abs(y - dy).max() / max(1.0, np.abs(dy).max())), "runs": 1}
        del K, Ln, xn
    else:
        out["numpy"] = {"status": "skipped", "message": "m > --numpy-max-m"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--numpy-max-m", type=int, default=1 << 30)
    ap.add_argument("--bench-json", default=None, help="file whose last JSON line is the output of `python bench.py --full` of this session")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_backend_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    dev = torch.device("cuda", 0)
    torch.ones(1, device=dev)
    bench_ref = {}
    if a.bench_json and os.path.exists(a.bench_json):
        lines = [ln for ln in open(a.bench_json).read().splitlines() if ln.startswith("{")]
        if lines:
            b = json.loads(lines[-1])
            bench_ref = {"roofline_frac": (b.get("roofline") or {}).get("frac"), "solve_gbs": (b.get("solve_roofline") or {}).get("achieved")}
    for shp in a.shapes.split(","):
        m, n = (int(v) for v in shp.lower().split("x"))
        line = json.dumps(run(m, n, a, torch, dev, bench_ref))
        print(line, flush=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
