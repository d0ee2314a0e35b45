"""What tlpk_set_values / tlpk_ipm_reload save against a fresh handle, on config C4 and on the north-star instance (workloads.py).

Per workload, written to profiles/set_values_bench.json (one JSON document; also printed line by line):
  create        wall time of KKT.setup (tlpk_create: host analyse + upload) and of the first update!
  first call    tlpk_set_values including the build and upload of the maps
  steady state  tlpk_set_values from a host pointer and tlpk_set_values_device (tlpk_stats.ms_last_set_values: HIP events around the
                refresh kernels), medians; next to them the byte model  8 nnzA + n_pairs (2*4 + 8) + 2*8 nnzA  (read nzval; per product two
                positions read, one product written; Tx and Px written), the rate it implies, its fraction of the 6.29 TB/s a device-to-device
                copy reaches on this GPU, and tlpk_stats.set_values_bytes
  conditions    ms_analyse is the same before and after (no analyse phase in a refresh; run with TLPK_TIMING=1 to see that no
                "[tlpk analyse]" line appears after the create), refresh + update! against create + update!
  end to end    DeviceHSD on LP1, then reload(A = R A, b = R b) for a positive diagonal R (row scaling keeps the optimum) and optimize again:
                setup and reload times, iteration counts, relative difference of the objectives
    python tools/set_values_bench.py [--only c4,north_star] [--reps 10] [--no-lp]
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

COPY_RATE = 6.29e12          # bytes/s of a device-to-device copy on one MI355X (read + write counted)


def median(v):
    return float(np.median(np.asarray(v, dtype=float)))


def kkt_part(name, A, row_block, reps, torch, dev):
    import tulip_jl_amd as tk
    from workloads import kernel_inputs
    m, n = A.shape
    th, rp, rd, _, _ = kernel_inputs(m, n, 7, "mid")
    rng = np.random.default_rng(11)
    out = {"workload": name, "m": m, "n": n, "nnzA": int(A.nnz)}
    t0 = time.perf_counter()
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=0, row_block=row_block))
    out["create_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    tk.update(kkt, th, rp, rd)
    out["first_update_s"] = time.perf_counter() - t0
    st = kkt.stats()
    out.update(ms_analyse=st["ms_analyse"], n_pairs=int(st["n_pairs"]), device_bytes_before=int(st["device_bytes"]))
    nz = [rng.standard_normal(A.nnz) for _ in range(2)]
    t0 = time.perf_counter()
    tk.set_values(kkt, nz[0])
    out["first_set_values_s"] = time.perf_counter() - t0
    st = kkt.stats()
    out.update(set_values_bytes=int(st["set_values_bytes"]), device_bytes_after=int(st["device_bytes"]))
    wall, dev_ms = [], []
    for r in range(reps):
        t0 = time.perf_counter()
        tk.set_values(kkt, nz[r & 1])
        wall.append(1e3 * (time.perf_counter() - t0))
        dev_ms.append(kkt.stats()["ms_last_set_values"])
    out.update(host_pointer_wall_ms=median(wall), host_pointer_device_ms=median(dev_ms))
    d_nz = [torch.from_numpy(v).to(dev) for v in nz]
    torch.cuda.synchronize()
    wall, dev_ms = [], []
    for r in range(reps):
        t0 = time.perf_counter()
        tk.set_values_device(kkt, d_nz[r & 1].data_ptr(), A.nnz)
        kkt.sync()
        wall.append(1e3 * (time.perf_counter() - t0))
        dev_ms.append(kkt.stats()["ms_last_set_values"])
    model = 8 * A.nnz + st["n_pairs"] * (2 * 4 + 8) + 2 * 8 * A.nnz
    rate = model / (1e-3 * median(dev_ms))
    out.update(device_pointer_wall_ms=median(wall), device_pointer_device_ms=median(dev_ms), model_bytes=int(model),
               achieved_bytes_per_s=rate, fraction_of_copy_rate=rate / COPY_RATE)
    t0 = time.perf_counter()
    tk.set_values(kkt, A.data)
    tk.update(kkt, th, rp, rd)
    out["refresh_plus_update_s"] = time.perf_counter() - t0
    out["create_plus_update_s"] = out["create_s"] + out["first_update_s"]
    out["ratio_create_over_refresh"] = out["create_plus_update_s"] / out["refresh_plus_update_s"]
    st = kkt.stats()
    out.update(ms_analyse_after=st["ms_analyse"], device_bytes_end=int(st["device_bytes"]))
    kkt.close()
    return out


def lp_part(name, A, row_block):
    from tulip_jl_amd.hsd_device import DeviceHSD
    m, n = A.shape
    rng = np.random.default_rng(20260927)
    xs = rng.uniform(0.0, 1.0, n) * (rng.random(n) < 0.6)
    b = A @ xs
    ys = rng.standard_normal(m)
    c = A.T @ ys + rng.uniform(0.0, 1.0, n) * (xs == 0.0)
    l = np.zeros(n); u = np.full(n, np.inf)
    out = {"workload": name, "part": "DeviceHSD"}
    t0 = time.perf_counter()
    opt = DeviceHSD(A, b, c, l, u, device=0, row_block=row_block)
    out["setup_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    opt.optimize()
    out.update(optimize_s=time.perf_counter() - t0, status=opt.status, iterations=opt.niter, objective=opt.primal_objective)
    r = rng.uniform(0.5, 2.0, m)
    A2 = sp.csc_matrix(sp.diags(r) @ A); A2.sort_indices()
    bytes0 = opt.kkt.stats()["device_bytes"]
    t0 = time.perf_counter()
    opt.reload(A=A2, b=r * b)
    out["reload_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    opt.optimize()
    out.update(reload_optimize_s=time.perf_counter() - t0, reload_status=opt.status, reload_iterations=opt.niter, reload_objective=opt.primal_objective,
               objective_rel_diff=abs(opt.primal_objective - out["objective"]) / (1 + abs(out["objective"])),
               device_bytes_grew_by=int(opt.kkt.stats()["device_bytes"] - bytes0), set_values_bytes=int(opt.kkt.stats()["set_values_bytes"]))
    opt.kkt.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="c4,north_star")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-lp", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_values_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    dev = torch.device("cuda", 0)
    torch.ones(1, device=dev)
    from workloads import block_angular_lp
    res = []
    for name in a.only.split(","):
        A, rb = block_angular_lp(100, 20000, 10000, 1000, 4, 0.5, ineq=True) if name == "north_star" else block_angular_lp()
        for part in ([kkt_part(name, A, rb, a.reps, torch, dev)] + ([] if a.no_lp else [lp_part(name, A, rb)])):
            print(json.dumps(part), flush=True)
            res.append(part)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/set_values_bench.py", "copy_rate_bytes_per_s": COPY_RATE, "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
