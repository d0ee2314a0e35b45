"""The matrix-free family after k = 1, 2, 3 iterations, entry by entry against long double (tests/krylov_reference.py, whose docstring is the
specification: the pair (v, e), the rule |device - v| <= 2 e, the model of the gather and its ten planted defects).

tests/test_krylov.py, test_krylov_k2.py and test_krylov_sqd.py compare CONVERGED solves with LAPACK to the stopping tolerance; tests/test_krylov_family.py
pins the branches of the shared gather (krylov_spmv.hpp) with digests recorded from the code itself.  Neither can see one dropped row of the second round
of a capped grid or a 65th long row that is skipped.  Here every case is the smallest that reaches one edge of that code, every handle (CG without and
with Jacobi, MINRES without and with Jacobi, TriCG) runs with itmax = k, and dx, dy, krylov_resid0, krylov_resid are held against the rule;
krylov_iters == k.  Every check runs on two drivers: "cpu", the float64 model of the gather (GatherModel), and "gpu", the device.

  1x1, 1x5, fixture          one partial wave.  The Krylov space is exhausted after a step or two: only the k of KS below are well-posed (the guard
                             asserts that the restatement's residual before step k is above the stopping tolerance and that its bound is resolved)
  127x255, 128x256, 129x257  one workgroup short by one, exact, one over: 128 rows / 256 columns per 1024-thread workgroup of k_cg_rows, k_mr_op, k_tc_op,
                             64 columns per workgroup of k_cg_cols, 32 rows per workgroup of the Jacobi kernels
  lens                       600 x 600; rows of exactly 0, 1, 7, 8, 9, 17, 511, 512, 513, 514 entries and columns of 0, 1, 3, 4, 5, 9, 511, 512, 513, 514
  long64, long65, long129    700 x 700 with 64, 65, 129 full rows and columns: the workgroups of the long lists take one trip each; the first one two;
                             one three and the rest two
  round1, round2             32768 x 65536 fills the capped row and column grids exactly; 32769 x 65537 is a second round with one live item
  vec2                       65537 x 70000: CG's order-m vector kernels make a second grid-stride trip with one live entry
  k2full, k2over             21845 x 43691 and 21845 x 43692: n + m = 65536 and 65537 for the vector kernels of MINRES and TriCG
The big cases run with k = 2 only.  Lines "KRYS <method> <case> k=<k> worst |dev - r| / 2e = ... (at entry ...)" are printed before anything is asserted;
profiles/krylov_step_checks.txt holds those of the MI355X."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import krylov_reference as kr
import tulip_jl_amd as tk
from helpers import ipm_like_data, kkt_residuals, random_lp_matrix

GPU = pytest.param("gpu", marks=pytest.mark.gpu)
DRIVERS = ["cpu", GPU]
# handle -> (K1 / K2, the restatement, the preconditioner, the arguments of KrylovBackend)
METHODS = {
    "cg": ("K1", "cg", None, dict(method="cg")),
    "cg-jacobi": ("K1", "cg", "jacobi", dict(method="cg", precond="jacobi")),
    "minres": ("K2", "minres", None, dict(method="minres")),
    "minres-jacobi": ("K2", "minres", "jacobi", dict(method="minres", precond="jacobi")),
    "tricg": ("K2", "tricg", None, dict(method="tricg")),
}
K1_HANDLES, K2_HANDLES = ["cg", "cg-jacobi"], ["minres", "minres-jacobi", "tricg"]
ROW_LENS = [0, 1, 7, 8, 9, 17, 511, 512, 513, 514]          # 0, 1, LANES - 1, LANES, LANES + 1, 2 LANES + 1 (8 lanes), the neighbours of CG_LONG
COL_LENS = [0, 1, 3, 4, 5, 9, 511, 512, 513, 514]           # the same with 4 lanes


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def _two_per_column(m, n, seed):
    """m x n, two distinct rows per column, N(0, 1) values (random_lp_matrix draws column by column: seconds at this size)"""
    rng = np.random.default_rng(seed)
    r0 = rng.integers(0, m, n)
    r1 = (r0 + 1 + rng.integers(0, m - 1, n)) % m
    A = sp.csc_matrix((rng.standard_normal(2 * n), (np.concatenate([r0, r1]), np.tile(np.arange(n), 2))), shape=(m, n))
    A.sort_indices()
    return A


def _lens():
    """600 x 600, three entries per column; rows 0 .. 9 and columns 0 .. 9 are then emptied and refilled outside that 10 x 10 corner with exactly
    ROW_LENS[r] and COL_LENS[c] entries"""
    rng = np.random.default_rng(5)
    A = random_lp_matrix(600, 600, 3, 5).toarray()
    A[:10, :] = 0.0; A[:, :10] = 0.0
    for r, L in enumerate(ROW_LENS):
        A[r, 10 + rng.choice(590, size=L, replace=False)] = rng.standard_normal(L)
    for c, L in enumerate(COL_LENS):
        A[10 + rng.choice(590, size=L, replace=False), c] = rng.standard_normal(L)
    return A


def _many_long(count):
    """tests/test_krylov_family.py's manylong with `count` full rows and columns"""
    rng = np.random.default_rng(7)
    A = random_lp_matrix(700, 700, 3, 7).toarray()
    A[:count, :] = rng.standard_normal((count, 700))
    A[:, :count] = rng.standard_normal((700, count))
    return A


MATRICES = {
    "1x1": lambda: random_lp_matrix(1, 1, 1, 1),
    "1x5": lambda: random_lp_matrix(1, 5, 1, 1),
    "fixture": lambda: np.array([[1.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 1.0]]),
    "127x255": lambda: random_lp_matrix(127, 255, 3, 1),
    "128x256": lambda: random_lp_matrix(128, 256, 3, 1),
    "129x257": lambda: random_lp_matrix(129, 257, 3, 1),
    "lens": _lens,
    "long64": lambda: _many_long(64),
    "long65": lambda: _many_long(65),
    "long129": lambda: _many_long(129),
    "round1": lambda: _two_per_column(32768, 65536, 1),
    "round2": lambda: _two_per_column(32769, 65537, 1),
    "vec2": lambda: _two_per_column(65537, 70000, 1),
    "k2full": lambda: _two_per_column(21845, 43691, 1),
    "k2over": lambda: _two_per_column(21845, 43692, 1),
}
SMALL = ["1x1", "1x5", "fixture", "127x255", "128x256", "129x257", "lens", "long64", "long65", "long129"]
# the k of a (case, handle) where not 1, 2, 3: the last step before the Krylov space is exhausted (K1 on one row, or with S = 2 I: one step)
KS = {("1x1", "cg"): [1], ("1x1", "cg-jacobi"): [1], ("1x5", "cg"): [1], ("1x5", "cg-jacobi"): [1], ("fixture", "cg"): [1], ("fixture", "cg-jacobi"): [1],
      ("1x1", "minres"): [1, 2], ("1x1", "minres-jacobi"): [1, 2], ("1x1", "tricg"): [1], ("1x5", "tricg"): [1], ("fixture", "tricg"): [1, 2]}
BIG = [(case, h) for case in ("round1", "round2") for h in METHODS] + [("vec2", h) for h in K1_HANDLES] + [(case, h) for case in ("k2full", "k2over") for h in K2_HANDLES]
RUNS = [(case, h) for case in SMALL for h in METHODS] + BIG


def ks_of(case, handle):
    return [2] if (case, handle) in BIG else KS.get((case, handle), [1, 2, 3])


@functools.lru_cache(maxsize=None)
def matrix(name):
    A = sp.csc_matrix(MATRICES[name]())
    A.sort_indices()
    return A


def data(name):
    m, n = matrix(name).shape
    return ipm_like_data(m, n, 1, "unit")


@functools.lru_cache(maxsize=None)
def lengths(name):
    A = matrix(name)
    return np.diff(A.tocsr().indptr), np.diff(A.indptr)


def check_premise(name):
    """the case reaches the edge it is there for"""
    A = matrix(name)
    m, n = A.shape
    rows, cols = lengths(name)
    gk1, gk2 = kr.geometry(rows, cols, True), kr.geometry(rows, cols, False)
    per_r, per_c = kr.OP_THREADS // kr.ROW_LANES, kr.OP_THREADS // kr.COL_LANES          # 128 rows, 256 columns per workgroup of the capped grids
    if name in ("1x1", "1x5", "fixture"):
        assert (m, n) == {"1x1": (1, 1), "1x5": (1, 5), "fixture": (2, 4)}[name] and gk2["g_rows"] == gk2["g_cols"] == gk2["g_vec"] == 1
    elif name in ("127x255", "128x256", "129x257"):
        want = {"127x255": 1, "128x256": 1, "129x257": 2}[name]
        assert (m - per_r, n - per_c) == {"127x255": (-1, -1), "128x256": (0, 0), "129x257": (1, 1)}[name]
        assert gk2["g_rows"] == gk2["g_cols"] == gk1["g_rows"] == want and rows.max() <= kr.CG_LONG and cols.max() <= kr.CG_LONG
        assert -(-n * kr.COL_LANES // kr.CG_THREADS) == {"127x255": 4, "128x256": 4, "129x257": 5}[name]          # k_cg_cols: 64 columns per workgroup
        assert -(-m * kr.ROW_LANES // kr.CG_THREADS) == {"127x255": 4, "128x256": 4, "129x257": 5}[name]          # Jacobi: 32 rows per workgroup
    elif name == "lens":
        assert rows[:10].tolist() == ROW_LENS and cols[:10].tolist() == COL_LENS and rows[10:].max() < 32 and cols[10:].max() < 32
        assert gk2["long_rows"].tolist() == [8, 9] and gk2["long_cols"].tolist() == [8, 9]
    elif name in ("long64", "long65", "long129"):
        count = int(name[4:])
        assert (rows > kr.CG_LONG).sum() == count == (cols > kr.CG_LONG).sum() and gk2["g_lrows"] == gk2["g_lcols"] == gk1["g_lrows"] == min(count, 64)
        trips = sorted(len(range(w, count, 64)) for w in range(min(count, 64)))
        assert (trips[0], trips[-2], trips[-1]) == {64: (1, 1, 1), 65: (1, 1, 2), 129: (2, 2, 3)}[count]
    elif name in ("round1", "round2"):
        assert rows.max() <= kr.CG_LONG and cols.max() <= kr.CG_LONG
        assert gk2["g_rows"] == gk2["g_cols"] == gk1["g_rows"] == kr.CG_MAX_SLOTS
        assert (m - 256 * per_r, n - 256 * per_c) == ((0, 0) if name == "round1" else (1, 1))
    elif name == "vec2":
        assert rows.max() <= kr.CG_LONG and gk1["g_vec"] == kr.CG_MAX_SLOTS and m - kr.CG_MAX_SLOTS * kr.CG_THREADS == 1
    else:
        assert rows.max() <= kr.CG_LONG and gk2["g_vec"] == kr.CG_MAX_SLOTS and n + m - kr.CG_MAX_SLOTS * kr.CG_THREADS == (0 if name == "k2full" else 1)


@functools.lru_cache(maxsize=None)
def restated(case, handle, arith):
    """the snapshots after iterations 1 .. max k of the case, in long double (the reference: computed once, shared, never changed) or float64"""
    _, method, precond, _ = METHODS[handle]
    return kr.STEPS[method](matrix(case), *data(case), precond=precond, k=max(ks_of(case, handle)), arith=getattr(kr, arith))


def reference(case, handle, k):
    return restated(case, handle, "LongDouble")[k - 1]


# ---------------------------------------------------------------------------------------------------------------------------------
# the drivers and the rule
# ---------------------------------------------------------------------------------------------------------------------------------
def solve(kind, case, handle, k, mut=None):
    """-> dx, dy, stats of one create / update / solve with itmax = k"""
    system, method, precond, kw = METHODS[handle]
    A = matrix(case)
    th, rp, rd, xp, xd = data(case)
    if kind == "cpu":
        mdl = kr.GatherModel(A, method, precond, itmax=k, mut=mut)
        mdl.update(th, rp, rd)
        dx, dy = mdl.solve(xp, xd)
        return dx, dy, mdl.stats
    assert mut is None
    kkt = tk.setup(A, tk.K1() if system == "K1" else tk.K2(), tk.KrylovBackend(device=0, itmax=k, **kw))
    tk.update(kkt, th, rp, rd)
    dx = np.zeros(A.shape[1]); dy = np.zeros(A.shape[0])
    tk.solve(dx, dy, kkt, xp, xd)
    st = kkt.stats()
    kkt.close()
    return dx, dy, st


def ratio(got, ref):
    """|got - v| / 2e, entry by entry; e = 0: 0 where got == v and inf elsewhere"""
    d = np.abs(np.atleast_1d(np.asarray(got, dtype=kr.LD)) - np.atleast_1d(ref.v))
    e = 2 * np.atleast_1d(ref.e)
    out = np.where(d == 0, 0.0, np.inf)
    np.divide(d, e, out=out, where=e > 0)
    return out.astype(np.float64)


def worst_of(dx, dy, st, ref):
    """-> (worst ratio, where) over dx, dy, krylov_resid0, krylov_resid"""
    best = (-1.0, "-")
    for name, got in (("dx", dx), ("dy", dy), ("resid0", st["krylov_resid0"]), ("resid", st["krylov_resid"])):
        r = ratio(got, ref[name])
        r = np.where(np.isnan(r), np.inf, r)
        if r.size and r.max() > best[0]:
            best = (float(r.max()), f"{name}[{int(r.argmax())}]" if name[0] == "d" else name)
    return best


def f64_ratio(case, handle, k):
    snap = restated(case, handle, "Float64")[k - 1]
    return worst_of(snap["dx"], snap["dy"], dict(krylov_resid0=snap["resid0"], krylov_resid=snap["resid"]), reference(case, handle, k))


# ---------------------------------------------------------------------------------------------------------------------------------
# guards (CPU): a violation here is a bad input or a bad bound, not a device failure
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(MATRICES))
def test_case_reaches_its_edge(case):
    check_premise(case)


@pytest.mark.parametrize("case,handle", RUNS, ids=[f"{c}-{h}" for c, h in RUNS])
def test_float64_restatement_is_inside_the_bound(case, handle):
    """... and the solve is well-posed for every k used: the residual before step k is above the stopping tolerance even at the far end of its bound (the
    device cannot have stopped earlier, krylov_iters == k), and B has raised no BoundError"""
    snaps = restated(case, handle, "LongDouble")
    tol = kr.SQRT_EPS * (1.0 + float(snaps[0]["resid0"].v))
    for k in ks_of(case, handle):
        before = snaps[k - 2]["resid"] if k > 1 else snaps[0]["resid0"]
        assert float(before.v - 2 * before.e) > tol, f"bad test input: {case} {handle} is solved before step {k}"
        w, at = f64_ratio(case, handle, k)
        print(f"KRYS {handle} {case} k={k} float64 restatement: worst |f64 - r| / 2e = {w:.3g} (at entry {at})")
        assert w <= 1.0, "bad input or bad bound: the float64 restatement of the same formulas is outside 2e"
    if (case, handle) in KS:          # the k left out are left out for a reason: the solve has stopped, or the next step divides by a norm that is zero
        k = max(KS[case, handle])
        if float(snaps[k - 1]["resid"].v - 2 * snaps[k - 1]["resid"].e) > tol:
            _, method, precond, _ = METHODS[handle]
            with pytest.raises(kr.BoundError):
                kr.STEPS[method](matrix(case), *data(case), precond=precond, k=k + 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the checks, on both drivers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", DRIVERS)
@pytest.mark.parametrize("case,handle", RUNS, ids=[f"{c}-{h}" for c, h in RUNS])
def test_steps_against_long_double(case, handle, kind):
    check_premise(case)
    failures = []
    for k in ks_of(case, handle):
        ref = reference(case, handle, k)
        dx, dy, st = solve(kind, case, handle, k)
        w, at = worst_of(dx, dy, st, ref)
        fw, _ = f64_ratio(case, handle, k)
        print(f"KRYS {handle} {case} k={k} worst |dev - r| / 2e = {w:.3g} (at entry {at})   [{kind}; float64 restatement {fw:.3g}; iters {st['krylov_iters']}]")
        if not (w <= 1.0 and st["krylov_iters"] == k):
            failures.append((k, w, at, st["krylov_iters"]))
        if METHODS[handle][1] == "cg":          # the exit gather on its own: dx against D (A'dy - xi_d) from the dy the driver returned
            th, rp, _, _, xd = data(case)
            r = ratio(dx, kr.exit_gather(matrix(case), th, rp, xd, dy))
            print(f"KRYS {handle} {case} k={k} exit gather: worst |dx - D (A'dy - xi_d)| / 2e = {r.max():.3g} (at entry dx[{int(r.argmax())}])   [{kind}]")
            if not r.max() <= 1.0:
                failures.append((k, float(r.max()), f"exit dx[{int(r.argmax())}]", st["krylov_iters"]))
    assert not failures, f"(k, worst ratio, where, iterations): {failures}"


# ---------------------------------------------------------------------------------------------------------------------------------
# mutations (CPU): each planted defect breaks the rule on the case built for it, by a factor of at least 100 at k = 2
# ---------------------------------------------------------------------------------------------------------------------------------
MUTANTS = [("one_round", "round2", "cg"), ("one_round", "round2", "minres"), ("one_round", "round2", "tricg"),
           ("long_one_trip", "long65", "cg"), ("long_one_trip", "long65", "minres"), ("long_one_trip", "long129", "tricg"),
           ("lt_long", "lens", "cg"), ("lt_long", "lens", "minres-jacobi"), ("lt_long", "lens", "tricg"),
           ("short_513", "lens", "cg-jacobi"), ("short_513", "lens", "minres"), ("short_513", "lens", "tricg"),
           ("last_group", "129x257", "cg"), ("last_group", "129x257", "minres"), ("last_group", "1x5", "tricg"),
           ("lane_one_trip", "lens", "cg"), ("lane_one_trip", "lens", "minres"), ("lane_one_trip", "lens", "tricg"),
           ("vec_one_trip", "vec2", "cg"), ("vec_one_trip", "k2over", "minres"), ("vec_one_trip", "k2over", "tricg"),
           ("row_block_offset", "129x257", "minres"), ("row_block_offset", "fixture", "tricg"),
           ("long_no_acc", "long64", "cg"), ("long_no_acc", "long64", "minres"), ("long_no_acc", "long64", "tricg"),
           ("jacobi_no_long", "long64", "cg-jacobi"), ("jacobi_no_long", "lens", "minres-jacobi")]
SEEN = 100.0


def test_every_mutation_has_a_case():
    assert sorted({mu for mu, _, _ in MUTANTS}) == sorted(kr.MUTATIONS) and len(kr.MUTATIONS) == 10


@pytest.mark.parametrize("mut,case,handle", MUTANTS, ids=[f"{mu}-{c}-{h}" for mu, c, h in MUTANTS])
def test_mutation_breaks_the_rule(mut, case, handle):
    check_premise(case)
    for k in [k for k in ks_of(case, handle) if k >= 2 or ks_of(case, handle) == [1]]:
        ref = reference(case, handle, k)
        w0, _ = worst_of(*solve("cpu", case, handle, k), ref)
        w, at = worst_of(*solve("cpu", case, handle, k, mut=mut), ref)
        print(f"KRYS {handle} {case} k={k} mutation {mut}: worst |dev - r| / 2e = {w:.3g} (at entry {at}); without it {w0:.3g}")
        assert w0 <= 1.0
        assert w >= SEEN, "the bound is too loose to see the defect"


CAP = 300          # iterations allowed to the two full solves below; the sound one needs a fraction of it


def test_mutation_one_round_against_the_criteria_of_a_converged_solve_and_against_the_rule():
    """The gap this file closes, in the spirit of tests/test_backward_error.py's test_mutation_one_small_entry...: the second round of k_cg_rows is not
    run on round2 (row 32768 is never gathered).  The sound model's solve meets tests/test_krylov.py's test_solution -- |dy - dy*|2 <= ((sqrt(eps) +
    sqrt(eps) rho0) + g) sqrt(max M) / lambda_min(S) and the residual of the second block row.  MEASURED, and not what was expected of it: the
    defective solve does not slip through those criteria.  q[32768] keeps its old content, the operator is no longer symmetric, r[32768] never moves
    and the solve never meets its stopping rule (run to 2 m iterations it ends at |dy - dy*|2 = 3.2e17).  So the criteria of a converged solve WOULD
    see this defect -- on a matrix that reaches the second round, after hundreds of iterations.  None of the converged suites' matrices does (asserted
    below), and the one test that does reach it, test_krylov_family.py's rounds, compares with digests recorded from the code.  The rule sees it
    after two iterations, 1e9 times outside 2e."""
    import test_krylov
    for name in test_krylov.MATRICES:          # (test_krylov_k2.py and test_krylov_sqd.py take theirs from the same table)
        mm, nn = test_krylov.matrix(name).shape
        assert mm <= 256 * 128 and nn <= 256 * 256, f"{name} reaches the second round: the converged suites are not blind to it any more"
    case, handle = "round2", "cg"
    A = matrix(case)
    m, n = A.shape
    th, rp, rd, xp, xd = data(case)
    D = 1.0 / (th + rp)
    S = (A @ sp.diags(D) @ A.T + sp.diags(rd)).tocsc()
    b = xp + A @ (D * xd)
    dy_star, info = spla.cg(S, b, rtol=1e-15, atol=0.0, maxiter=500)
    assert info == 0 and np.linalg.norm(S @ dy_star - b) <= 1e-13 * np.linalg.norm(b)
    lam_min = float(rd.min())          # S = A D A' + Rd >= Rd; the criteria's lambda_min(S) is no smaller, their bound no larger
    verdicts = {}
    for mut in (None, "one_round"):
        mdl = kr.GatherModel(A, "cg", None, itmax=CAP, mut=mut)
        mdl.update(th, rp, rd)
        dx, dy = mdl.solve(xp, xd)
        it, rho0 = mdl.stats["krylov_iters"], mdl.stats["krylov_resid0"]
        s_inf = float(abs(S).sum(axis=1).max())
        g = 4.0 * it * kr.EPS * (s_inf * np.abs(dy).max() + np.abs(b).max()) * np.sqrt(m)
        bound = ((kr.SQRT_EPS + kr.SQRT_EPS * rho0) + g) / lam_min
        err = float(np.linalg.norm(dy - dy_star))
        _, r2 = kkt_residuals(A, th, rp, rd, xp, xd, dx, dy)
        a_inf = float(abs(A).sum(axis=1).max())
        r2_bound = 100 * kr.EPS * (np.abs(dx).max() * (th + rp).max() + a_inf * np.abs(dy).max() + np.abs(xd).max())
        w, at = worst_of(*solve("cpu", case, handle, 2, mut=mut), reference(case, handle, 2))
        print(f"KRYS {handle} {case} mutation {mut}: {it} iterations of at most {CAP}, |dy - dy*|2 = {err:.3e} (bound {bound:.3e}), r2 = {r2:.3e} (bound {r2_bound:.3e}); "
              f"k=2 worst |dev - r| / 2e = {w:.3g} (at entry {at})")
        verdicts[mut] = (it < CAP, err <= bound and r2 <= r2_bound, w)
    assert verdicts[None][0] and verdicts[None][1] and verdicts[None][2] <= 1.0
    assert not verdicts["one_round"][0] and not verdicts["one_round"][1]          # as measured: see the docstring
    assert verdicts["one_round"][2] >= SEEN
