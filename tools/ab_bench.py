#!/usr/bin/env python3
"""A/B of two builds of libtlpk.so on one GPU in one session (the protocol of profiles/ea_gather_bench.json and profiles/ea_form_bench.json):
`bench.py --gpus 1 --steps 20 --warmup 5 --repeats 3 [--workload W]`, the parent's build (TLPK_LIB) and this tree's build alternating, --runs runs per
build and workload; optionally the vectors of `--dump-outputs` of both builds compared bitwise, and the roofline leg (`kernel_ms`) of both.

    python tools/ab_bench.py --parent-lib PATH/libtlpk.so --workloads c4,headline,pds --out profiles/NAME.json [--dump c4,headline] [--roofline]

Every bench.py run is a process of its own under a time limit; the first run that fails ends the script (nothing more is started on the GPU).
The result file is rewritten after every run, and merged with what it already holds, so that the legs can be collected by several invocations."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--gpus", "1", "--steps", "20", "--warmup", "5", "--repeats", "3"]
ROOFLINE = ["--full", "--no-cpu-baseline", "--no-headline", "--no-host-abi", "--no-small-lp", "--no-c3"]


def bench(lib, extra, limit):
    env = dict(os.environ)
    env.pop("TLPK_LIB", None)
    if lib:
        env["TLPK_LIB"] = lib
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "bench.py")] + BASE + extra
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"bench.py {' '.join(extra)} (lib={lib or 'this'}) ended with {r.returncode}: nothing more is run")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])


def summary(runs):
    med = [statistics.median(r) for r in runs]
    return {"ms_per_step": [round(m, 4) for m in med], "ms_per_step_runs": runs, "median": round(statistics.median(med), 4),
            "spread_max_minus_min": round(max(med) - min(med), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--this-lib", default=None, help="the build measured as `this` (default: the tree's own libtlpk.so)")
    ap.add_argument("--workloads", default="c4,headline,pds")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dump", default="", help="workloads whose --dump-outputs vectors are compared bitwise")
    ap.add_argument("--roofline", action="store_true", help="the per-kernel leg of c4, once per build")
    ap.add_argument("--limit", type=int, default=400, help="seconds per bench.py run")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    parent = os.path.abspath(a.parent_lib)
    this = os.path.abspath(a.this_lib) if a.this_lib else None
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}

    def save():
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for w in [x for x in a.workloads.split(",") if x]:
        extra = [] if w == "c4" else ["--workload", w]
        runs = {"parent": [], "this": []}
        for k in range(a.runs):
            for which, lib in (("parent", parent), ("this", this)):
                out = bench(lib, extra, a.limit)
                runs[which].append(out["ms_per_step_runs"])
                print(f"{w} run {k} {which}: {out['ms_per_step']:.4f} ms", flush=True)
                res[w] = {b: summary(r) for b, r in runs.items() if r}
                save()
        p, t = res[w]["parent"], res[w]["this"]
        res[w]["change_of_median_ms"] = round(t["median"] - p["median"], 4)
        res[w]["three_times_larger_spread"] = round(3 * max(p["spread_max_minus_min"], t["spread_max_minus_min"]), 4)
        save()
    for w in [x for x in a.dump.split(",") if x]:
        extra = [] if w == "c4" else ["--workload", w]
        with tempfile.TemporaryDirectory() as d:
            for which, lib in (("parent", parent), ("this", this)):
                bench(lib, extra + ["--dump-outputs", os.path.join(d, which)], a.limit)
            names = sorted(os.listdir(os.path.join(d, "parent")))
            same = names == sorted(os.listdir(os.path.join(d, "this"))) and all(
                np.array_equal(np.load(os.path.join(d, "parent", n)).view(np.uint64), np.load(os.path.join(d, "this", n)).view(np.uint64)) for n in names)
        res.setdefault("dumped_outputs", {})[w] = f"{len(names)} arrays of `--dump-outputs`, parent vs this: " + ("bitwise equal" if same else "DIFFERENT")
        print(w, res["dumped_outputs"][w], flush=True)
        save()
        if not same:
            raise SystemExit("dumped outputs differ")
    if a.roofline:
        leg = {"command": "bench.py " + " ".join(BASE[2:] + ROOFLINE)}
        for which, lib in (("parent", parent), ("this", this)):
            out = bench(lib, ROOFLINE, a.limit)
            leg[f"kernel_ms_{which}"] = out.get("kernel_ms")
            leg.setdefault("ms_per_step", {})[which] = out["ms_per_step"]
        res["roofline_leg_c4"] = leg
        save()


if __name__ == "__main__":
    main()
