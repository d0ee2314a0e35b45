"""What a skipped block still costs: update and solve times of a block-diagonal stack with K of its B blocks active (tlpk_block_skip).

Inputs: B in {64, 512} copies of the standard-form matrix of tests/golden/stair25.mps stacked into one handle (row_block = copy index), mid-IPM
update data (theta_inv = 10^U(-3, 3), regP = regD = 1e-4).  Every block is factorised once without a mask; then, for K = B, B/2, B/8 and 1, the
blocks K .. B - 1 are skipped and `reps` updates and `reps` solves are timed through tlpk_stats (ms_last_update / ms_last_solve: device time between
the events that bracket the call), median reported.  The row "no mask" is the handle before any mask was set (the null-pointer path of the
kernels); K = B is the same work with the mask's bytes read.  K = 1 is the floor that launches and empty workgroups leave: the schedule, the
grids and the task lists are those of the whole stack whatever the mask says.
Written to profiles/block_skip_bench.json and printed line by line.  Every B runs in a child process of its own under `timeout`.

    python tools/block_skip_bench.py [--sizes 64,512] [--reps 7] [--system K1]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
LIMIT_S = 240


def worker(B, reps, system):
    import scipy.sparse as sp
    import tulip_jl_amd as tk
    from helpers import DevBuf, ipm_like_data
    from tulip_jl_amd.problem import read_free_mps, standard_form
    A1 = sp.csc_matrix(standard_form(read_free_mps(os.path.join(ROOT, "tests", "golden", "stair25.mps"))).A)
    A = sp.block_diag([A1] * B, format="csc")
    A.sort_indices()
    rb = np.repeat(np.arange(B), A1.shape[0]).astype(np.int64)
    kkt = tk.setup(A, tk.K2() if system == "K2" else tk.K1(), tk.Backend(device=0, row_block=rb))
    m, n = A.shape
    th, rp, rd, xp, xd = (DevBuf(v) for v in ipm_like_data(m, n, 1, regime="mid"))
    dx, dy = DevBuf(n), DevBuf(m)
    med = lambda v: float(np.median(np.asarray(v, dtype=float)))                         # noqa: E731

    def timed():
        up, so = [], []
        for r in range(reps + 1):                                                        # (the first pair is a warm-up: graph capture, first touch)
            kkt.update_device(th.ptr, rp.ptr, rd.ptr)
            up.append(kkt.stats()["ms_last_update"])
            kkt.solve_device(dx.ptr, dy.ptr, xp.ptr, xd.ptr)
            so.append(kkt.stats()["ms_last_solve"])
        return med(up[1:]), med(so[1:])

    st = kkt.stats()
    out = {"B": B, "system": system, "m": m, "n": n, "fronts": int(len(kkt.symbolic("front_ns"))), "launches_update": int(st["launches_update"]),
           "launches_solve": int(st["launches_solve"]), "reps": reps, "rows": []}
    u, s = timed()
    out["rows"].append({"K": B, "mask": "none", "ms_update": u, "ms_solve": s})
    for K in sorted({B, max(B // 2, 1), max(B // 8, 1), 1}, reverse=True):
        tk.block_skip(kkt, (np.arange(B) >= K).astype(np.uint8))
        u, s = timed()
        out["rows"].append({"K": K, "mask": "set", "ms_update": u, "ms_solve": s})
    tk.block_skip(kkt, None)
    out["skip_bytes"] = int(kkt.symbolic("skip_bytes")[0])
    full, floor = out["rows"][1], out["rows"][-1]
    out["floor_share_update"] = floor["ms_update"] / full["ms_update"]
    out["floor_share_solve"] = floor["ms_solve"] / full["ms_solve"]
    kkt.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,512")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--system", default="K1")
    ap.add_argument("--worker", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_skip_bench.json"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.reps, a.system)
    res = []
    for B in (int(s) for s in a.sizes.split(",")):
        p = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--worker", str(B), "--reps", str(a.reps),
                            "--system", a.system], capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"B = {B}: exit status {p.returncode}; nothing more is started on the GPU\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}", flush=True)
            break
        res.append(json.loads(line[0][len("RESULT "):]))
        print(json.dumps(res[-1]), flush=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/block_skip_bench.py", "results": res}, f, indent=1)
    return 0 if len(res) == len(a.sizes.split(",")) else 1


if __name__ == "__main__":
    sys.exit(main())
