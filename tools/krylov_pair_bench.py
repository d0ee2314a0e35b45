"""tlpk_solve2_device on the matrix-free handles (DESIGN.md section 1b'''''''): a pair of right-hand sides through one sequence of launches against the same
two right-hand sides through two solves, on the matrix of ONE config-C4 block (5000 x 10000) and of EIGHT C4 blocks with their linking rows (41000 x 80000),
workloads.py.  Written to profiles/krylov_pair_bench.json (one JSON document; also printed).

  per method      CG and CG + Jacobi (K1), MINRES and MINRES + Jacobi, TriCG (K2): two handles on the same matrix in the same process, one created with
                  the pair on and one under TLPK_KRYLOV_PAIR=0 (the two-solve path, which is the code path of before the pair existed).  Solves that cannot
                  converge (atol = rtol = 1e-300) with itmax = --iters, so that both legs run the same number of rounds.  The two legs ALTERNATE, --reps
                  times after a warm-up of each; wall time of tlpk_solve2_device + tlpk_sync around device buffers.  Reported: the median of each leg, the
                  spread of each leg over its own repeats (min, max), pair / two solves, microseconds per round of the pair, and the bytes of a round
                  of the pair
                      2 x (single model) - (what the two right-hand sides share)
                  with the single models of tools/krylov_bench.py, krylov_k2_bench.py, krylov_sqd_bench.py and, shared, A's values and indices in both
                  passes (24 nnz), the pointer arrays (8 N) and the diagonals (CG: D, Rd, 16 m more with Jacobi; MINRES: E, Rd, 8 N more with Jacobi;
                  TriCG: W and 1 / W in the three kernels, 32 N): A counted once, the vectors twice.  Achieved bytes/s = model / time and its fraction of
                  the 6.29 TB/s of a streaming copy.  The outputs of the two legs are compared for equality.
  DeviceHSD       a C4-block LP through the device-resident HSD loop on a CG + Jacobi handle with the pair on and off, alternating: solve time per
                  interior-point iteration, with statuses and iteration counts equal (--hsd-iters interior-point iterations, --hsd-itmax Krylov
                  iterations per solve at most: a bound on the run, the late systems of an interior-point run are beyond Jacobi-CG)

    python tools/krylov_pair_bench.py [--iters 400] [--reps 7]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12          # bytes/s of a device-to-device copy on one MI355X (read + write counted)
HANDLES = (("cg", "K1", dict(method="cg")), ("cg-jacobi", "K1", dict(method="cg", precond="jacobi")), ("minres", "K2", dict(method="minres")),
           ("minres-jacobi", "K2", dict(method="minres", precond="jacobi")), ("tricg", "K2", dict(method="tricg")))


class DevBuf:
    """device doubles through the HIP runtime the library is linked against"""
    _hip = None

    def __init__(self, data_or_len):
        import tulip_jl_amd._lib as L
        if DevBuf._hip is None:
            L.lib()
            h = ctypes.CDLL("libamdhip64.so")
            h.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
            h.hipFree.argtypes = [ctypes.c_void_p]
            h.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
            DevBuf._hip = h
        a = np.zeros(int(data_or_len)) if np.isscalar(data_or_len) else np.ascontiguousarray(data_or_len, dtype=np.float64)
        self.n = a.size
        p = ctypes.c_void_p()
        assert DevBuf._hip.hipMalloc(ctypes.byref(p), max(8 * self.n, 8)) == 0
        self.ptr = p.value
        assert DevBuf._hip.hipMemcpy(self.ptr, a.ctypes.data, 8 * self.n, 1) == 0

    def get(self):
        out = np.empty(self.n)
        assert DevBuf._hip.hipMemcpy(out.ctypes.data, self.ptr, 8 * self.n, 2) == 0
        return out


def models(name, m, n, nnz):
    """(bytes of an iteration of one solve, bytes the two right-hand sides of a pair share)"""
    N = n + m
    jac = name.endswith("jacobi")
    if name.startswith("cg"):
        return 40 * nnz + 24 * n + 104 * m + (16 * m if jac else 0), 24 * nnz + 8 * N + 8 * n + 8 * m + (16 * m if jac else 0)
    if name.startswith("minres"):
        return 40 * nnz + 112 * N + (16 * N if jac else 0), 24 * nnz + 8 * N + 8 * N + (8 * N if jac else 0)
    return 40 * nnz + 152 * N + 8 * m, 24 * nnz + 8 * N + 32 * N


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def one(workload, A, iters, reps):
    import tulip_jl_amd as tk
    m, n = A.shape
    nnz = int(A.nnz)
    rng = np.random.default_rng(5)
    rhs = [(rng.standard_normal(m), rng.standard_normal(n)) for _ in range(2)]
    ones_n, ones_m = np.ones(n), np.ones(m)
    out = {"workload": workload, "m": m, "n": n, "nnzA": nnz, "rounds": iters, "reps": reps, "handles": {}}
    for name, system, kw in HANDLES:
        legs = {}
        for leg, knob in (("pair", None), ("two_solves", "0")):
            os.environ.pop("TLPK_KRYLOV_PAIR", None)
            if knob is not None:
                os.environ["TLPK_KRYLOV_PAIR"] = knob
            kkt = tk.setup(A, tk.K1() if system == "K1" else tk.K2(), tk.KrylovBackend(device=0, itmax=iters, atol=1e-300, rtol=1e-300, **kw))
            tk.update(kkt, ones_n, ones_n, ones_m)
            legs[leg] = {"kkt": kkt, "in": [DevBuf(v) for r in rhs for v in r], "out": [DevBuf(n), DevBuf(m), DevBuf(n), DevBuf(m)], "wall_ms": []}
        os.environ.pop("TLPK_KRYLOV_PAIR", None)

        def run(L):
            i, o = L["in"], L["out"]
            t0 = time.perf_counter()
            L["kkt"].solve2_device(o[0].ptr, o[1].ptr, i[0].ptr, i[1].ptr, o[2].ptr, o[3].ptr, i[2].ptr, i[3].ptr)
            return 1e3 * (time.perf_counter() - t0)

        for L in legs.values():          # warm-up: code objects, the second set of the pair
            run(L); run(L)
        for _ in range(reps):            # alternating
            for L in legs.values():
                L["wall_ms"].append(run(L))
        info = [int(v) for v in legs["pair"]["kkt"].symbolic("krylov_pair")]
        off = [int(v) for v in legs["two_solves"]["kkt"].symbolic("krylov_pair")]
        assert info[0] == reps + 2 and info[1] == 0 and info[2] == info[3] == iters and off[0] == 0, (info, off)
        equal = all((a.get().tobytes() == b.get().tobytes()) for a, b in zip(legs["pair"]["out"], legs["two_solves"]["out"]))
        single, shared = models(name, m, n, nnz)
        model = 2 * single - shared
        p, t = spread(legs["pair"]["wall_ms"]), spread(legs["two_solves"]["wall_ms"])
        us = 1e3 * p["median"] / iters
        r = {"pair_wall_ms": p, "two_solves_wall_ms": t, "pair_over_two_solves": p["median"] / t["median"],
             "two_solves_spread_max_over_min": t["max"] / t["min"], "outputs_equal": bool(equal),
             "launches_pair": int(legs["pair"]["kkt"].stats()["launches_solve"]), "launches_last_of_two_solves": int(legs["two_solves"]["kkt"].stats()["launches_solve"]),
             "pair_us_per_round": us, "two_solves_us_per_round": 1e3 * t["median"] / iters, "model_bytes_per_round_pair": model,
             "model_bytes_per_iteration_single": single, "achieved_bytes_per_s": model / (1e-6 * us), "fraction_of_copy_rate": model / (1e-6 * us) / COPY_RATE,
             "device_bytes_pair": int(legs["pair"]["kkt"].stats()["device_bytes"]), "device_bytes_two_solves": int(legs["two_solves"]["kkt"].stats()["device_bytes"])}
        for L in legs.values():
            L["kkt"].close()
        print(json.dumps({workload: {name: r}}), flush=True)
        out["handles"][name] = r
    return out


def hsd(A, hsd_iters, itmax, reps):
    import tulip_jl_amd as tk
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

    runs = {"pair": [], "two_solves": []}
    for rep in range(reps + 1):          # (the first round of both legs is the warm-up)
        for leg, knob in (("pair", "1"), ("two_solves", "0")):
            os.environ["TLPK_KRYLOV_PAIR"] = knob
            opt = DeviceHSD(A, b, c, l, u, options=Few(), backend=tk.KrylovBackend(method="cg", precond="jacobi", itmax=itmax))
            t0 = time.perf_counter()
            opt.optimize()
            sec = time.perf_counter() - t0
            if rep:
                runs[leg].append({"status": opt.status, "iterations": int(opt.niter), "objective": float(opt.primal_objective).hex(),
                                  "ms_per_iteration": 1e3 * sec / max(opt.niter, 1), "paired": int(opt.kkt.symbolic("krylov_pair")[0]),
                                  "unsolved": int(opt.kkt.symbolic("krylov_unsolved")[0])})
            opt.kkt.close()
    os.environ.pop("TLPK_KRYLOV_PAIR", None)
    p, t = runs["pair"], runs["two_solves"]
    same = all((a["status"], a["iterations"], a["objective"]) == (b_["status"], b_["iterations"], b_["objective"]) for a, b_ in zip(p, t))
    ps, ts = spread([r["ms_per_iteration"] for r in p]), spread([r["ms_per_iteration"] for r in t])
    return {"workload": "c4_one_block LP, DeviceHSD, CG + Jacobi", "hsd_iterations_limit": hsd_iters, "krylov_itmax": itmax, "status": p[0]["status"],
            "iterations": p[0]["iterations"], "status_iterations_objective_equal": bool(same), "paired_solves": p[0]["paired"], "unsolved": p[0]["unsolved"],
            "pair_ms_per_iteration": ps, "two_solves_ms_per_iteration": ts, "pair_over_two_solves": ps["median"] / ts["median"],
            "two_solves_spread_max_over_min": ts["max"] / ts["min"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--hsd-iters", type=int, default=8)
    ap.add_argument("--hsd-itmax", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "krylov_pair_bench.json"))
    a = ap.parse_args()
    import tulip_jl_amd as tk
    if tk._lib.lib().tlpk_device_count() < 1:
        raise SystemExit("needs a GPU")
    from workloads import block_angular_lp
    doc = {"tool": "tools/krylov_pair_bench.py", "copy_rate_bytes_per_s": COPY_RATE, "results": []}

    def save():
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)

    A1 = None
    for name, kw in (("c4_one_block", dict(nblocks=1, m0=0)), ("c4_eight_blocks", dict(nblocks=8))):
        A, _ = block_angular_lp(**kw)
        A1 = A if A1 is None else A1
        doc["results"].append(one(name, A, a.iters, a.reps))
        save()
    doc["device_hsd"] = hsd(A1, a.hsd_iters, a.hsd_itmax, max(3, a.reps // 2))
    print(json.dumps(doc["device_hsd"]), flush=True)
    save()


if __name__ == "__main__":
    main()
