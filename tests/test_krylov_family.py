"""Bit identity of the matrix-free family (conjugate gradients on K1, MINRES and TriCG on K2) across changes that do not mean to alter arithmetic.

The three methods share one sparse gather (tulip.jl_amd/csrc/krylov_spmv.hpp) and one solve driver (tlpk_api.cpp: krylov_run).  Every case below is solved by
five handles -- CG without and with Jacobi, MINRES without and with Jacobi, TriCG -- and the SHA-256 of the bytes of dx and of dy, the iteration count, the
outcome, the two residual norms (as hex floats) and the launch count of the solve are compared FOR EQUALITY with tests/golden/krylov_family_digests.json.
There is no tolerance: the digests pin the summation order documented in krylov_reduce.hpp (a fixed shuffle tree per row, column and workgroup, the partial
sums added in slot order), which is what makes two solves of the same data bit-identical.  Whether the branches these cases reach compute the RIGHT sums
is checked in tests/test_krylov_steps.py, against long double after one, two and three iterations.

The fixture is re-recorded only by a change that MEANS to alter arithmetic, or by a compiler change; it names the `hipcc --version` it was recorded with.
A change that must keep the arithmetic (a refactoring) records it from a build of its PARENT commit -- a copy of the parent tree with this one file added,
the same hipcc -- and never from the code under test:

    python tests/test_krylov_family.py --record tests/golden/krylov_family_digests.json

The cases are the smallest ones that reach each branch of the shared code (CG_LONG = 512 entries, CG_MAX_LONG = 64 workgroups for the long lists, at most
256 workgroups of 1024 threads for the short rows, 8 lanes each, and for the short columns, 4 lanes each):
  fixture, r1x5      one partial wave
  long600            one long row, one long column, one empty row, one empty column
  manylong           70 long rows and 70 long columns of 700 entries: the workgroups of the long lists take more than one trip
  rounds             m = 33000 > 256 * 128 and n = 66000 > 256 * 256: the capped short-row and short-column grids make two rounds and the vector kernels
                     grid-stride; 40 iterations, ending at itmax is as good as converging here
  r40x10 "mid"       the itmax exit
  r30x50 "mid"       long convergence
  r500, chunk 1,2    TLPK_CG_CHUNK=1,2: several trips through the driver loop; everything but the launch count equals the default chunking"""
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import functools
import hashlib
import json
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import tulip_jl_amd as tk
from helpers import ipm_like_data, random_lp_matrix
from test_krylov_sqd import data as table_data, matrix as table_matrix

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "krylov_family_digests.json")
# (K1 / K2, the arguments of KrylovBackend)
METHODS = {
    "cg": ("K1", dict(method="cg")),
    "cg-jacobi": ("K1", dict(method="cg", precond="jacobi")),
    "minres": ("K2", dict(method="minres")),
    "minres-jacobi": ("K2", dict(method="minres", precond="jacobi")),
    "tricg": ("K2", dict(method="tricg")),
}
# case -> (matrix, regime, itmax (0: the default), TLPK_CG_CHUNK (None: the default))
CASES = {
    "fixture": ("fixture", "unit", 0, None),
    "r1x5": ("r1x5", "unit", 0, None),
    "long600": ("long600", "unit", 0, None),
    "manylong": ("manylong", "unit", 0, None),
    "rounds": ("rounds", "unit", 40, None),
    "r40x10-mid": ("r40x10", "mid", 0, None),
    "r30x50-mid": ("r30x50", "mid", 0, None),
    "r500": ("r500", "unit", 0, None),
    "r500-chunk1,2": ("r500", "unit", 0, "1,2"),
}
KEYS = ("dx", "dy", "krylov_iters", "krylov_converged", "krylov_resid0", "krylov_resid", "launches_solve")


def _many_long():
    """700 x 700, 3 random entries per column, then rows 0 .. 69 and columns 0 .. 69 made full"""
    rng = np.random.default_rng(7)
    A = random_lp_matrix(700, 700, 3, 7).toarray()
    A[:70, :] = rng.standard_normal((70, 700))
    A[:, :70] = rng.standard_normal((700, 70))
    A = sp.csc_matrix(A); A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name == "manylong":
        return _many_long()
    if name == "rounds":
        return random_lp_matrix(33000, 66000, 3, 1)
    return table_matrix(name)


def data(name, regime):
    if name in ("manylong", "rounds"):
        m, n = matrix(name).shape
        return ipm_like_data(m, n, 1, regime)
    return table_data(name, regime)


def _sha(v):
    return hashlib.sha256(np.ascontiguousarray(v, dtype=np.float64).tobytes()).hexdigest()


def solve_record(case, method):
    """one create / update / solve on the device -> the record the fixture stores.  The caller has set or unset TLPK_CG_CHUNK (read at create)."""
    name, regime, itmax, chunk = CASES[case]
    assert os.environ.get("TLPK_CG_CHUNK") == chunk
    system, kw = METHODS[method]
    A = matrix(name)
    m, n = A.shape
    kkt = tk.setup(A, tk.K1() if system == "K1" else tk.K2(), tk.KrylovBackend(device=0, itmax=itmax, **kw))
    th, rp, rd, xp, xd = data(name, regime)
    tk.update(kkt, th, rp, rd)
    dx = np.zeros(n); dy = np.zeros(m)
    tk.solve(dx, dy, kkt, xp, xd)
    st = kkt.stats()
    kkt.close()
    return {"dx": _sha(dx), "dy": _sha(dy), "krylov_iters": int(st["krylov_iters"]), "krylov_converged": int(st["krylov_converged"]),
            "krylov_resid0": float(st["krylov_resid0"]).hex(), "krylov_resid": float(st["krylov_resid"]).hex(), "launches_solve": int(st["launches_solve"])}


@functools.lru_cache(maxsize=None)
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.gpu          # (needs none itself: it guards the inputs and the fixture of the comparisons below and runs with them)
def test_fixture_covers_every_case_and_names_its_compiler():
    fx = recorded()
    assert "version" in fx["hipcc_version"].lower()
    assert sorted(fx["cases"]) == sorted(CASES)
    for case, per_method in fx["cases"].items():
        assert sorted(per_method) == sorted(METHODS), case
        for rec in per_method.values():
            assert sorted(rec) == sorted(KEYS), case
    # the inputs reach the branches they are there for
    lens = lambda A: (np.diff(A.indptr), np.diff(A.tocsr().indptr))
    cols, rows = lens(matrix("manylong"))
    assert (cols > 512).sum() >= 70 > 64 and (rows > 512).sum() >= 70
    cols, rows = lens(matrix("long600"))
    assert (cols > 512).sum() == 1 and (rows > 512).sum() == 1 and (cols == 0).sum() == 1 and (rows == 0).sum() == 1


@pytest.mark.gpu
@pytest.mark.parametrize("method", sorted(METHODS))
@pytest.mark.parametrize("case", [c for c in CASES if CASES[c][3] is None])
def test_digests_equal_the_recorded_ones(case, method, monkeypatch):
    monkeypatch.delenv("TLPK_CG_CHUNK", raising=False)
    got, want = solve_record(case, method), recorded()["cases"][case][method]
    print(f"{case} {method}: {got}")
    assert got == want, f"recorded with {recorded()['hipcc_version']!r}"


@pytest.mark.gpu
@pytest.mark.parametrize("method", sorted(METHODS))
def test_chunking_changes_the_launch_count_only(method, monkeypatch):
    monkeypatch.setenv("TLPK_CG_CHUNK", "1,2")
    got = solve_record("r500-chunk1,2", method)
    print(f"r500 chunk 1,2 {method}: {got}")
    assert got == recorded()["cases"]["r500-chunk1,2"][method]
    default = recorded()["cases"]["r500"][method]
    for key in KEYS[:-1]:
        assert got[key] == default[key], key
    assert got["krylov_iters"] > 3          # chunks of 1, 2, 2, ...: more than two trips through the driver loop


def _record(path):
    ver = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    out = {"hipcc_version": " | ".join(s.strip() for s in ver[:2]), "cases": {}}
    for case in CASES:
        os.environ.pop("TLPK_CG_CHUNK", None)
        if CASES[case][3]:
            os.environ["TLPK_CG_CHUNK"] = CASES[case][3]
        out["cases"][case] = {method: solve_record(case, method) for method in sorted(METHODS)}
        print(case, json.dumps(out["cases"][case]), flush=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        raise SystemExit("usage: python tests/test_krylov_family.py --record PATH")
    _record(sys.argv[2])
