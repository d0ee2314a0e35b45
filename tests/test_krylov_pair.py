"""tlpk_solve2_device on a matrix-free handle: both right-hand sides through ONE sequence of launches (DESIGN.md section 1b''''''').

The contract is bit identity per right-hand side: dx, dy, iteration count, outcome, resid0 and resid of each one are those of tlpk_solve_device on that
right-hand side alone on the same handle, whichever of the two stops first and however it stops.  Every comparison below is `==` on bytes and integers;
there is no tolerance.  Five handles: CG without and with Jacobi (K1), MINRES without and with Jacobi, TriCG (K2).  The matrices and data are those of
tests/test_krylov_family.py, and right-hand side A of the branch cases must also reproduce the digests recorded there, which pins the pair path to the
arithmetic of the single solve as it was before the pair existed.  Right-hand side B is cos / sin of the index.

"krylov_pair" (tlpk_symbolic_get): [paired solves since create, fallbacks to two solves since create, iterations of number 0, of number 1, outcome code of
number 0, of number 1 (1 solved, 2 itmax, 3 breakdown), rounds of launches enqueued by the last pair]; "krylov_pair_resid" (tlpk_symbolic_get_f64):
[resid0, resid of number 0, resid0, resid of number 1]."""
import os

import numpy as np
import pytest

import tulip_jl_amd as tk
from tulip_jl_amd import _lib
from helpers import DevBuf
from test_krylov_family import CASES, METHODS, _sha, data, matrix, recorded

pytestmark = pytest.mark.gpu

SOLVED, ITMAX, BREAKDOWN = 1, 2, 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BRANCH_CASES = ["fixture", "r1x5", "long600", "manylong", "r40x10-mid", "r30x50-mid", "rounds"]


def handle(method, A, itmax=0, **extra):
    system, kw = METHODS[method]
    return tk.setup(A, tk.K1() if system == "K1" else tk.K2(), tk.KrylovBackend(device=0, itmax=itmax, **kw, **extra))


def rhs_b(m, n):
    return np.cos(np.arange(m)), np.sin(np.arange(n))


def _record(kkt):
    st = kkt.stats()
    return {"iters": int(st["krylov_iters"]), "converged": int(st["krylov_converged"]), "resid0": float(st["krylov_resid0"]).hex(),
            "resid": float(st["krylov_resid"]).hex(), "launches": int(st["launches_solve"])}


def single(kkt, rhs):
    """tlpk_solve_device -> (dx, dy, record)"""
    xp, xd = rhs
    b_xp, b_xd, b_dx, b_dy = DevBuf(xp), DevBuf(xd), DevBuf(kkt.n), DevBuf(kkt.m)
    kkt.solve_device(b_dx.ptr, b_dy.ptr, b_xp.ptr, b_xd.ptr)
    return b_dx.get(), b_dy.get(), _record(kkt)


def pair(kkt, rhs0, rhs1):
    """tlpk_solve2_device -> ((dx0, dy0), (dx1, dy1), the stats of the handle behind it, "krylov_pair", "krylov_pair_resid")"""
    same = rhs0 is rhs1
    i0 = [DevBuf(rhs0[0]), DevBuf(rhs0[1])]
    i1 = i0 if same else [DevBuf(rhs1[0]), DevBuf(rhs1[1])]          # (inputs may alias each other)
    o = [DevBuf(kkt.n), DevBuf(kkt.m), DevBuf(kkt.n), DevBuf(kkt.m)]
    kkt.solve2_device(o[0].ptr, o[1].ptr, i0[0].ptr, i0[1].ptr, o[2].ptr, o[3].ptr, i1[0].ptr, i1[1].ptr)
    return (o[0].get(), o[1].get()), (o[2].get(), o[3].get()), _record(kkt), [int(v) for v in kkt.symbolic("krylov_pair")], \
        [float(v).hex() for v in _lib.symbolic_array_f64(kkt._h, "krylov_pair_resid")]


def same_bytes(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def assert_pair_is_singles(kkt, rhs0, rhs1, s0, s1, what=""):
    """one pair on kkt against the single solves s0, s1 = (dx, dy, record) of its two right-hand sides on the same handle; returns "krylov_pair" """
    total0, unsolved0, pairs0 = kkt.stats()["krylov_iters_total"], int(kkt.symbolic("krylov_unsolved")[0]), int(kkt.symbolic("krylov_pair")[0])
    p0, p1, rec, info, resid = pair(kkt, rhs0, rhs1)
    print(f"{what}: singles {s0[2]} {s1[2]}; pair {info} {resid}, stats {rec}")
    for got, want, r in ((p0, s0, 0), (p1, s1, 1)):
        assert same_bytes(got[0], want[0]) and same_bytes(got[1], want[1]), f"{what}: dx / dy of number {r}"
        assert info[2 + r] == want[2]["iters"], f"{what}: iterations of number {r}"
        assert (info[4 + r] == SOLVED) == bool(want[2]["converged"]) and info[4 + r] in (SOLVED, ITMAX, BREAKDOWN), f"{what}: outcome of number {r}"
        assert resid[2 * r] == want[2]["resid0"] and resid[2 * r + 1] == want[2]["resid"], f"{what}: residuals of number {r}"
    # the statistics read as after the two solves one behind the other; the launches are those of the longer one
    assert {k: rec[k] for k in ("iters", "converged", "resid0", "resid")} == {k: s1[2][k] for k in ("iters", "converged", "resid0", "resid")}, what
    assert rec["launches"] == max(s0[2]["launches"], s1[2]["launches"]), what
    assert kkt.stats()["krylov_iters_total"] == total0 + s0[2]["iters"] + s1[2]["iters"], what
    assert int(kkt.symbolic("krylov_unsolved")[0]) == unsolved0 + (1 - s0[2]["converged"]) + (1 - s1[2]["converged"]), what
    assert info[0] == pairs0 + 1 and info[1] == 0, what
    return info


ATOL = float(np.sqrt(np.finfo(np.float64).eps))          # krylov_atol = krylov_rtol = 0 -> sqrt(eps)


def quick_rhs(method, A, th, rp, rd):
    """A right-hand side that meets the stopping rule after 1 .. 3 iterations, whatever the conditioning: the rule is resid <= atol + rtol resid0, and a
    right-hand side scaled until resid0 is just above atol needs only the reduction that k <= 3 iterations give.  The iterations are linear in the
    right-hand side, so a probe at scale 1 (handles with itmax = 1, 2, 3: resid0 and the residual after k iterations) fixes the scale that puts atol at the
    geometric mean of the two.  A residual that does not fall by 3 % within 3 iterations (TriCG's is not monotone) rules a candidate out; the candidates are
    B, e_0 in xi_p, e_0 in xi_d, and K2 times [dx; dy] = [e_0; 0], that is xi_p = A e_0, xi_d = -E e_0.  The last one is there for TriCG: its solution has
    dy = 0 and dx along E^-1 xi_d, the first Lanczos vector u_1, so the Galerkin iterate of the FIRST iteration is the solution and the solve meets the rule
    at scale 1.  The caller asserts the premise from the single solve on its own handle."""
    m, n = A.shape
    e_p, e_d = np.zeros(m), np.zeros(n)
    e_p[0] = 1.0; e_d[0] = 1.0
    k_e0 = (np.asarray(A[:, [0]].todense()).ravel().astype(np.float64), -(th[0] + rp[0]) * e_d)
    for name, cand in (("B", rhs_b(m, n)), ("e0 in xi_p", (e_p, np.zeros(n))), ("e0 in xi_d", (np.zeros(m), e_d)), ("K2 [e0; 0]", k_e0)):
        for k in (1, 2, 3):
            probe = handle(method, A, itmax=k)
            tk.update(probe, th, rp, rd)
            rec = single(probe, cand)[2]
            probe.close()
            r0, rk = float.fromhex(rec["resid0"]), float.fromhex(rec["resid"])
            print(f"quick_rhs {method} {name} itmax {k}: resid0 {r0:.3e} resid {rk:.3e} converged {rec['converged']}")
            if rec["converged"] and rec["iters"] >= 1:
                return cand
            if 0.0 < rk < 0.97 * r0:
                scale = ATOL / float(np.sqrt(rk * r0))
                return cand[0] * scale, cand[1] * scale
    raise AssertionError("bad test input: no candidate's residual falls within 3 iterations")


# 1 ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", sorted(METHODS))
@pytest.mark.parametrize("case", BRANCH_CASES)
def test_pair_equals_singles_on_the_branch_cases(case, method, monkeypatch):
    monkeypatch.delenv("TLPK_CG_CHUNK", raising=False)
    monkeypatch.delenv("TLPK_KRYLOV_PAIR", raising=False)
    name, regime, itmax, _ = CASES[case]
    A = matrix(name)
    m, n = A.shape
    th, rp, rd, xp, xd = data(name, regime)
    kkt = handle(method, A, itmax=itmax)
    tk.update(kkt, th, rp, rd)
    ra, rb = (xp, xd), rhs_b(m, n)
    sa, sb = single(kkt, ra), single(kkt, rb)
    want = recorded()["cases"][case][method]
    for order, (r0, r1, s0, s1) in (("(A, B)", (ra, rb, sa, sb)), ("(B, A)", (rb, ra, sb, sa))):
        assert_pair_is_singles(kkt, r0, r1, s0, s1, f"{case} {method} {order}")
    # number 0 of (A, B) once more, against the recorded digests of the single solve
    (dx, dy), _, _, info, resid = pair(kkt, ra, rb)
    got = {"dx": _sha(dx), "dy": _sha(dy), "krylov_iters": info[2], "krylov_converged": int(info[4] == SOLVED), "krylov_resid0": resid[0], "krylov_resid": resid[1]}
    assert got == {k: want[k] for k in got}, f"recorded with {recorded()['hipcc_version']!r}"
    kkt.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", sorted(METHODS))
@pytest.mark.parametrize("case", ["r500", "r30x50-mid"])
def test_different_ends(case, method, monkeypatch):
    """chunks of 1, 2, 2, ... rounds: the two right-hand sides end in different chunks, and the launches go on for the longer one over the parked one.
    The second right-hand side is quick_rhs's, which ends within 3 iterations (unscaled, B and A take the same number of iterations on r500, and on
    r30x50 "mid" both run to itmax without a preconditioner).  That the counts differ by 3 or more is asserted from the two single solves."""
    monkeypatch.setenv("TLPK_CG_CHUNK", "1,2")
    monkeypatch.delenv("TLPK_KRYLOV_PAIR", raising=False)
    name, regime, itmax, _ = CASES[case]
    A = matrix(name)
    m, n = A.shape
    th, rp, rd, xp, xd = data(name, regime)
    kkt = handle(method, A, itmax=itmax)
    tk.update(kkt, th, rp, rd)
    ra, rb = (xp, xd), quick_rhs(method, A, th, rp, rd)
    sa, sb = single(kkt, ra), single(kkt, rb)
    print(f"{case} {method}: A {sa[2]}, B {sb[2]}")
    assert abs(sa[2]["iters"] - sb[2]["iters"]) >= 3, "bad test input: the two solves must end in different chunks"
    (rl, sl), (rs, ss) = ((ra, sa), (rb, sb)) if sa[2]["iters"] > sb[2]["iters"] else ((rb, sb), (ra, sa))
    assert sl[2]["launches"] > ss[2]["launches"]
    info = assert_pair_is_singles(kkt, rl, rs, sl, ss, f"{case} {method} (long, short)")          # the longer one first: launches_solve is NOT that of the last solve
    assert kkt.stats()["launches_solve"] == sl[2]["launches"]
    assert info[6] > ss[2]["iters"] and info[6] >= sl[2]["iters"]                                # rounds enqueued: past the end of the shorter one
    assert_pair_is_singles(kkt, rs, rl, ss, sl, f"{case} {method} (short, long)")
    kkt.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", sorted(METHODS))
def test_one_right_hand_side_settled_by_init(method, monkeypatch):
    monkeypatch.delenv("TLPK_CG_CHUNK", raising=False)
    monkeypatch.delenv("TLPK_KRYLOV_PAIR", raising=False)
    A = matrix("r500")
    m, n = A.shape
    th, rp, rd, xp, xd = data("r500", "unit")
    kkt = handle(method, A)
    tk.update(kkt, th, rp, rd)
    ra, rz = (xp, xd), (np.zeros(m), np.zeros(n))
    sa, sz = single(kkt, ra), single(kkt, rz)
    assert sz[2]["iters"] == 0 and sz[2]["converged"] == 1 and not sz[0].any() and not sz[1].any()
    for r0, r1, s0, s1, z in ((ra, rz, sa, sz, 1), (rz, ra, sz, sa, 0)):
        info = assert_pair_is_singles(kkt, r0, r1, s0, s1, f"{method} zero at {z}")
        assert info[2 + z] == 0 and info[4 + z] == SOLVED and info[2 + (1 - z)] == sa[2]["iters"] > 0
    kkt.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", sorted(METHODS))
def test_one_breaks_at_init_one_solves(method, monkeypatch):
    monkeypatch.delenv("TLPK_CG_CHUNK", raising=False)
    monkeypatch.delenv("TLPK_KRYLOV_PAIR", raising=False)
    A = matrix("r500")          # (every handle solves it: r30x50 "mid" runs to itmax without a preconditioner)
    m, n = A.shape
    th, rp, rd, xp, xd = data("r500", "unit")
    kkt = handle(method, A)
    tk.update(kkt, th, rp, rd)
    bp, bd = rhs_b(m, n)
    bp = bp.copy(); bp[m // 2] = np.nan
    ra, rn = (xp, xd), (bp, bd)
    sa, sn = single(kkt, ra), single(kkt, rn)
    assert sa[2]["converged"] == 1 and sn[2]["converged"] == 0 and sn[2]["iters"] == 0
    for r0, r1, s0, s1, z in ((ra, rn, sa, sn, 1), (rn, ra, sn, sa, 0)):
        unsolved = int(kkt.symbolic("krylov_unsolved")[0])
        info = assert_pair_is_singles(kkt, r0, r1, s0, s1, f"{method} NaN at {z}")
        assert info[4 + z] == BREAKDOWN and info[2 + z] == 0 and info[4 + (1 - z)] == SOLVED
        assert int(kkt.symbolic("krylov_unsolved")[0]) == unsolved + 1
    kkt.close()


@pytest.mark.parametrize("method", ["cg", "cg-jacobi"])
def test_one_breaks_in_the_step_one_solves(method, monkeypatch):
    """an empty row with Rd = 0 there and a right-hand side supported on it: p'q = 0 in the first k_cg_step, which parks that right-hand side alone"""
    monkeypatch.delenv("TLPK_CG_CHUNK", raising=False)
    monkeypatch.delenv("TLPK_KRYLOV_PAIR", raising=False)
    A = matrix("long600")
    m, n = A.shape
    rows = np.diff(A.tocsr().indptr)
    assert (rows == 0).sum() == 1
    i0 = int(np.flatnonzero(rows == 0)[0])
    th, rp, rd, xp, xd = data("long600", "unit")
    rd = rd.copy(); rd[i0] = 0.0
    xp = xp.copy(); xp[i0] = 0.0                      # A leaves the singular row alone and solves
    ep = np.zeros(m); ep[i0] = 1.0
    kkt = handle(method, A)
    tk.update(kkt, th, rp, rd)
    ra, rbad = (xp, xd), (ep, np.zeros(n))
    sa, sbad = single(kkt, ra), single(kkt, rbad)
    assert sa[2]["converged"] == 1 and sa[2]["iters"] > 1 and sbad[2]["converged"] == 0 and sbad[2]["iters"] == 0
    for r0, r1, s0, s1, z in ((ra, rbad, sa, sbad, 1), (rbad, ra, sbad, sa, 0)):
        unsolved = int(kkt.symbolic("krylov_unsolved")[0])
        info = assert_pair_is_singles(kkt, r0, r1, s0, s1, f"{method} breakdown at {z}")
        assert info[4 + z] == BREAKDOWN and info[4 + (1 - z)] == SOLVED
        assert int(kkt.symbolic("krylov_unsolved")[0]) == unsolved + 1
    kkt.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", sorted(METHODS))
def test_itmax_small(method, monkeypatch):
    """itmax = 3: one right-hand side meets the rule within 3 iterations (quick_rhs; asserted from its single solve), the other stops at itmax"""
    monkeypatch.delenv("TLPK_CG_CHUNK", raising=False)
    monkeypatch.delenv("TLPK_KRYLOV_PAIR", raising=False)
    A = matrix("r30x50")
    m, n = A.shape
    th, rp, rd, xp, xd = data("r30x50", "mid")
    kkt = handle(method, A, itmax=3)
    tk.update(kkt, th, rp, rd)
    ra = (xp, xd)
    sa = single(kkt, ra)
    assert sa[2]["converged"] == 0 and sa[2]["iters"] == 3
    rq = quick_rhs(method, A, th, rp, rd)
    sq = single(kkt, rq)
    print(f"{method}: A {sa[2]}, quick {sq[2]}")
    assert sq[2]["converged"] == 1 and 1 <= sq[2]["iters"] <= 3, "bad test input: the quick right-hand side must meet the rule within 3 iterations"
    for r0, r1, s0, s1, z in ((ra, rq, sa, sq, 0), (rq, ra, sq, sa, 1)):
        info = assert_pair_is_singles(kkt, r0, r1, s0, s1, f"{method} itmax at {z}")
        assert info[4 + z] == ITMAX and info[2 + z] == 3 and info[4 + (1 - z)] == SOLVED
    kkt.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", sorted(METHODS))
def test_state_stays_clean(method, monkeypatch):
    monkeypatch.delenv("TLPK_CG_CHUNK", raising=False)
    monkeypatch.delenv("TLPK_KRYLOV_PAIR", raising=False)
    A = matrix("r500")
    m, n = A.shape
    th, rp, rd, xp, xd = data("r500", "unit")
    th2 = th * 1.7 + 0.1
    A2 = A.copy(); A2.data = A.data * np.linspace(0.5, 1.5, A.nnz)
    ra, rb = (xp, xd), rhs_b(m, n)

    def fresh(M, theta):
        f = handle(method, M)
        tk.update(f, theta, rp, rd)
        out = single(f, ra), single(f, rb)
        f.close()
        return out

    fa, fb = fresh(A, th)
    fa2, fb2 = fresh(A, th2)
    fa3, fb3 = fresh(A2, th)
    strip = lambda s: (s[0], s[1], {k: v for k, v in s[2].items()})
    kkt = handle(method, A)
    tk.update(kkt, th, rp, rd)
    assert_pair_is_singles(kkt, ra, rb, strip(fa), strip(fb), f"{method} first pair")
    total = kkt.stats()["krylov_iters_total"]
    assert total == fa[2]["iters"] + fb[2]["iters"]
    s = single(kkt, ra)                                                      # a single solve behind a pair
    assert same_bytes(s[0], fa[0]) and same_bytes(s[1], fa[1]) and s[2] == fa[2]
    assert kkt.stats()["krylov_iters_total"] == total + fa[2]["iters"]
    assert_pair_is_singles(kkt, ra, rb, strip(fa), strip(fb), f"{method} pair behind a single solve")
    assert_pair_is_singles(kkt, rb, ra, strip(fb), strip(fa), f"{method} two pairs in a row")
    assert_pair_is_singles(kkt, ra, ra, strip(fa), strip(fa), f"{method} the same right-hand side twice")
    tk.update(kkt, th2, rp, rd)                                              # other values
    assert_pair_is_singles(kkt, ra, rb, strip(fa2), strip(fb2), f"{method} pair behind an update")
    tk.set_values(kkt, A2)                                                   # a reload on the analysed pattern
    tk.update(kkt, th, rp, rd)
    assert_pair_is_singles(kkt, ra, rb, strip(fa3), strip(fb3), f"{method} pair behind set_values")
    kkt.close()


# 7 ---------------------------------------------------------------------------------------------------------------------------------------------------------
def krylov_bytes(method, A):
    """the memory gate of a matrix-free handle (tlpk_api.cpp: krylov_bytes): what the handle needs WITHOUT the second set of a pair"""
    m, n = A.shape
    per = {"cg": (80, 136), "cg-jacobi": (80, 136), "minres": (144, 176), "minres-jacobi": (144, 176), "tricg": (136, 168)}[method]
    return 36 * A.nnz + per[0] * n + per[1] * m + 65536


@pytest.mark.parametrize("method", sorted(METHODS))
def test_the_knob_and_the_budget(method, monkeypatch):
    monkeypatch.delenv("TLPK_CG_CHUNK", raising=False)
    monkeypatch.delenv("TLPK_KRYLOV_PAIR", raising=False)
    A = matrix("r500")
    m, n = A.shape
    th, rp, rd, xp, xd = data("r500", "unit")
    ra, rb = (xp, xd), rhs_b(m, n)
    on = handle(method, A)
    tk.update(on, th, rp, rd)
    p0, p1, rec, info, resid = pair(on, ra, rb)
    assert info[0] == 1 and info[1] == 0
    on.close()
    monkeypatch.setenv("TLPK_KRYLOV_PAIR", "0")
    off = handle(method, A)
    monkeypatch.delenv("TLPK_KRYLOV_PAIR")
    tight = handle(method, A, mem_budget_bytes=krylov_bytes(method, A))      # fits the handle, not the second set
    for kkt, fallbacks in ((off, 0), (tight, 1)):
        tk.update(kkt, th, rp, rd)
        q0, q1, qrec, qinfo, _ = pair(kkt, ra, rb)
        assert same_bytes(q0[0], p0[0]) and same_bytes(q0[1], p0[1]) and same_bytes(q1[0], p1[0]) and same_bytes(q1[1], p1[1])
        assert qinfo[0] == 0 and qinfo[1] == fallbacks and qinfo[2:] == [0, 0, 0, 0, 0]
        assert {k: qrec[k] for k in ("iters", "converged", "resid0", "resid")} == {k: rec[k] for k in ("iters", "converged", "resid0", "resid")}
        kkt.close()


# 8 ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["cg-jacobi", "minres-jacobi", "tricg"])
def test_through_the_loop(method, monkeypatch):
    """DeviceHSD issues the h-system and the predictor as a pair every iteration (tlpk_ipm_hsolve_newton): with the pair on and off the run is the same, bit for bit"""
    from tulip_jl_amd.hsd_device import DeviceHSD
    from tulip_jl_amd.problem import read_free_mps, standard_form
    monkeypatch.delenv("TLPK_CG_CHUNK", raising=False)
    d = standard_form(read_free_mps(os.path.join(GOLDEN, "lpex_opt.mps")))
    system, kw = METHODS[method]
    runs = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("TLPK_KRYLOV_PAIR", knob)
        opt = DeviceHSD(d.A, d.b, d.c, d.l, d.u, c0=d.c0, objsense_min=d.objsense, system=system, backend=tk.KrylovBackend(**kw)).optimize()
        sol = opt.solution()
        runs[knob] = (opt.status, opt.niter, float(opt.primal_objective).hex(), float(opt.dual_objective).hex(), sol["x"].tobytes(), sol["y"].tobytes(), sol["s"].tobytes(),
                      float(opt.tau).hex(), float(opt.kappa).hex())
        info = [int(v) for v in opt.kkt.symbolic("krylov_pair")]
        print(f"{method} pair {knob}: {opt.status} in {opt.niter} iterations, z = {opt.primal_objective!r}, krylov_pair {info}")
        assert opt.status == "Trm_Optimal" and opt.timers.get("n_paired", 0) > 0
        assert (info[0] > 0) == (knob == "1") and info[1] == 0
    assert runs["1"] == runs["0"]
