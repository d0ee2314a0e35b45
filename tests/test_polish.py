"""Refinement on demand on the device: tlpk_polish_device / tlpk_polish2_device / tlpk_ipm_set_polish (include/tlpk.h; DESIGN.md section 1c').

What is pinned: on K1 the new call equals tlpk_options.refine_steps bit for bit; on K2 (which had no refinement) one step removes the error the solve
leaves in r1; the norms the call reports are those of the vectors (long double, within the rounding bound of the kernel's own sums); the residual
kernel at its block boundaries; a pair equals its two singles bit for bit, each system with its own verdicts; new values reach the K2 copies of A;
the loops with polish=k equal the loops on a refine=k handle; the refusals that need a device."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import tulip_jl_amd as tk
from helpers import DevBuf, block_angular, ipm_like_data, random_lp_matrix
from polish_reference import allowances, norms_ld
from test_polish_host import K2_INPUTS, k1_input, k2_input
from tulip_jl_amd import _lib

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def handle(A, system="K1", **kw):
    return tk.setup(A, tk.K2() if system == "K2" else tk.K1(), tk.Backend(device=0, **kw))


def solved(kkt, xp, xd):
    """dx, dy of tlpk_solve_device as host arrays (the handle is factored)."""
    bx, by, bp, bd = DevBuf(kkt.n), DevBuf(kkt.m), DevBuf(xp), DevBuf(xd)
    kkt.solve_device(bx.ptr, by.ptr, bp.ptr, bd.ptr)
    return bx.get(), by.get()


def polished(kkt, dx, dy, xp, xd, steps):
    """tlpk_polish_device on copies of (dx, dy): the corrected vectors and the report of system 0."""
    bx, by, bp, bd = DevBuf(dx), DevBuf(dy), DevBuf(xp), DevBuf(xd)
    kkt.polish_device(bx.ptr, by.ptr, bp.ptr, bd.ptr, steps=steps)
    rep = kkt.polish_report()
    assert rep["sides"][1] == dict.fromkeys(rep["sides"][1], 0)          # one system: the second block reads zero
    return bx.get(), by.get(), rep["sides"][0]


def polished2(kkt, s0, s1, steps):
    """tlpk_polish2_device on copies; s = (dx, dy, xp, xd).  The same right-hand side may be given twice (the inputs alias, the outputs never)."""
    same_rhs = s0[2] is s1[2] and s0[3] is s1[3]
    b0 = [DevBuf(s0[0]), DevBuf(s0[1]), DevBuf(s0[2]), DevBuf(s0[3])]
    b1 = [DevBuf(s1[0]), DevBuf(s1[1])] + (b0[2:] if same_rhs else [DevBuf(s1[2]), DevBuf(s1[3])])
    kkt.polish2_device(*[b.ptr for b in b0], *[b.ptr for b in b1], steps=steps)
    rep = kkt.polish_report()["sides"]
    return (b0[0].get(), b0[1].get(), rep[0]), (b1[0].get(), b1[1].get(), rep[1])


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def k1_case():
    if "k1" not in _cache:
        _cache["k1"] = (k1_input("late"), k1_input("mid")[1])
    return _cache["k1"]


# ---- 1. K1 equals the option ---------------------------------------------------------------------------------------------------------
def option_equals_polish(A, data, steps, **kw):
    th, rp, rd, xp, xd = data
    plain = handle(A, **kw)
    tk.update(plain, th, rp, rd)
    dx0, dy0 = solved(plain, xp, xd)
    out = []
    for s in steps:
        ref = handle(A, refine=s, **kw)
        tk.update(ref, th, rp, rd)
        rx, ry = solved(ref, xp, xd)
        want_rej = ref.stats()["refine_rejected"]
        ref.close()
        px, py, rep = polished(plain, dx0, dy0, xp, xd, s)
        print(f"steps {s}: option rejected {want_rej}; polish {rep}")
        assert same_bits(px, rx) and same_bits(py, ry)
        assert rep["rejected"] == want_rej and rep["asked"] == s and rep["accepted"] + rep["rejected"] <= s
        assert plain.stats()["refine_rejected"] == 0                      # tlpk_stats.refine_rejected is not touched
        out.append((px, py, rep))
    plain.close()
    return (dx0, dy0), out


@pytest.mark.parametrize("regime", ["late", "mid"])
def test_k1_polish_equals_the_refine_option_bit_for_bit(regime):
    (A, late), mid = k1_case()
    (dx0, _), out = option_equals_polish(A, late if regime == "late" else mid, (1, 2))
    if regime == "late":
        assert out[0][2]["accepted"] == 1 and not same_bits(out[0][0], dx0)      # (the comparison is not one of two unrefined solves)


def test_k1_dense_cols_and_row_block_handles_equal_the_option():
    from test_dense_cols import planted
    A, _ = planted(300, 700, 3, [150, 200], 5)
    m, n = A.shape
    option_equals_polish(A, ipm_like_data(m, n, 3, "late"), (1,), dense_cols="auto", dense_col_min=50)
    A, rb = block_angular(nblocks=4, mk=200, nk=400, m0=40, nnz_in=3, link_prob=0.5, seed=1)
    m, n = A.shape
    option_equals_polish(A, ipm_like_data(m, n, 3, "late"), (1,), row_block=rb)


# ---- 2. K2 accuracy ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,seed", K2_INPUTS)
def test_k2_one_step_removes_the_error_of_the_solve(m, n, seed):
    """Long double: |r1|inf(after) <= |r1|inf(before) / 100 (the CPU oracle gives >= 1.3e4: two orders are left for the device's ordering and summation),
    |r2|inf(after) <= 16 |r2|inf(before), one accepted step; three steps leave neither norm of the kept iterate above that after one."""
    A, data = k2_input(m, n, seed)
    th, rp, rd, xp, xd = data
    kkt = handle(A, "K2")
    tk.update(kkt, th, rp, rd)
    dx0, dy0 = solved(kkt, xp, xd)
    before = norms_ld(A, th, rp, rd, xp, xd, dx0, dy0)
    dx1, dy1, rep1 = polished(kkt, dx0, dy0, xp, xd, 1)
    after = norms_ld(A, th, rp, rd, xp, xd, dx1, dy1)
    dx3, dy3, rep3 = polished(kkt, dx0, dy0, xp, xd, 3)
    after3 = norms_ld(A, th, rp, rd, xp, xd, dx3, dy3)
    assert kkt.polish_report()["bytes"] > 0
    kkt.close()
    print(f"K2 {m} x {n}: |r1| {before[0]:.3e} -> {after[0]:.3e} -> (3 steps) {after3[0]:.3e}; |r2| {before[1]:.3e} -> {after[1]:.3e} -> {after3[1]:.3e}; {rep1}; {rep3}")
    assert rep1["accepted"] == 1 and rep1["rejected"] == 0
    assert after[0] <= before[0] / 100
    assert after[1] <= 16 * before[1]
    assert rep3["accepted"] >= 1 and rep3["accepted"] + rep3["rejected"] <= 3
    assert after3[0] <= after[0] and after3[1] <= after[1]


# ---- 3. / 4. the reported norms ------------------------------------------------------------------------------------------------------
def check_norms(A, data, xp, xd, vec_in, vec_out, rep, what):
    th, rp, rd = data
    for tag, (dx, dy), got in (("entry", vec_in, (rep["r1_in"], rep["r2_in"])), ("kept", vec_out, (rep["r1"], rep["r2"]))):
        want = norms_ld(A, th, rp, rd, xp, xd, dx, dy)
        tol = allowances(A, th, rp, rd, xp, xd, dx, dy)
        print(f"{what} {tag}: reported {got[0]:.6e}, {got[1]:.6e}; long double {want[0]:.6e}, {want[1]:.6e}; allowance {tol[0]:.2e}, {tol[1]:.2e}")
        assert abs(got[0] - want[0]) <= tol[0] and abs(got[1] - want[1]) <= tol[1], (what, tag)


@pytest.mark.parametrize("system", ["K1", "K2"])
def test_reported_norms_are_those_of_the_vectors(system):
    if system == "K1":
        (A, data), _ = k1_case()
    else:
        A, data = k2_input(*K2_INPUTS[0])
    th, rp, rd, xp, xd = data
    kkt = handle(A, system)
    tk.update(kkt, th, rp, rd)
    dx0, dy0 = solved(kkt, xp, xd)
    dx1, dy1, rep = polished(kkt, dx0, dy0, xp, xd, 1)
    kkt.close()
    assert rep["accepted"] == 1
    check_norms(A, (th, rp, rd), xp, xd, (dx0, dy0), (dx1, dy1), rep, system)


def edge_matrices():
    out = [("1x1", sp.csc_matrix(np.array([[2.5]]))),
           ("2x4", sp.csc_matrix(np.array([[1.0, 0, 1, 0], [0, 1, 0, 1]])))]           # the fixture of the reference's KKT tests
    for (m, n) in ((255, 257), (256, 256), (257, 255), (513, 300)):
        out.append((f"{m}x{n}", random_lp_matrix(m, n, 3, 100 + m)))
    B = random_lp_matrix(260, 300, 3, 9).tolil()
    B[17, :] = 0; B[:, 258] = 0                                                   # an empty row and an empty column
    B = B.tocsc(); B.eliminate_zeros(); B.sort_indices()
    assert B.getnnz(axis=1)[17] == 0 and B.getnnz(axis=0)[258] == 0
    out.append(("empty", B))
    F = random_lp_matrix(130, 300, 2, 10).tolil()
    F[64, :] = np.random.default_rng(3).standard_normal(300)                        # one row holding all n entries
    F = F.tocsc(); F.sort_indices()
    out.append(("fullrow", F))
    return out


@pytest.mark.parametrize("system", ["K1", "K2"])
@pytest.mark.parametrize("name,A", edge_matrices(), ids=[e[0] for e in edge_matrices()])
def test_residual_kernel_edge_shapes(name, A, system):
    """steps = 0 on arbitrary vectors: the norms as in the test above, dx and dy untouched bit for bit, no step counted."""
    m, n = A.shape
    th, rp, rd, xp, xd = ipm_like_data(m, n, 5, "mid")
    rng = np.random.default_rng(m + n)
    dx, dy = rng.standard_normal(n), rng.standard_normal(m)
    kkt = handle(A, system)
    tk.update(kkt, th, rp, rd)
    ox, oy, rep = polished(kkt, dx, dy, xp, xd, 0)
    kkt.close()
    assert same_bits(ox, dx) and same_bits(oy, dy)
    assert rep["asked"] == rep["accepted"] == rep["rejected"] == 0
    assert rep["r1"] == rep["r1_in"] and rep["r2"] == rep["r2_in"]
    check_norms(A, (th, rp, rd), xp, xd, (dx, dy), (dx, dy), rep, f"{system} {name}")


# ---- 5. pair equals singles ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("system", ["K1", "K2"])
def test_pair_equals_singles_bit_for_bit(system):
    if system == "K1":
        (A, data), _ = k1_case()
    else:
        A, data = k2_input(*K2_INPUTS[0])
    m, n = A.shape
    th, rp, rd, xp, xd = data
    rng = np.random.default_rng(12)
    xp2, xd2 = rng.standard_normal(m), rng.standard_normal(n)
    kkt = handle(A, system)
    tk.update(kkt, th, rp, rd)
    a = solved(kkt, xp, xd) + (xp, xd)
    b = solved(kkt, xp2, xd2) + (xp2, xd2)
    zero = (np.zeros(n), np.zeros(m), np.zeros(m), np.zeros(n))
    single = {}
    for steps in (1, 2):
        for tag, s in (("a", a), ("b", b), ("zero", zero)):
            single[tag, steps] = polished(kkt, *s, steps)
    assert single["a", 1][2]["accepted"] == 1

    def check(tag0, s0, tag1, s1, steps):
        got = polished2(kkt, s0, s1, steps)
        for tag, g in ((tag0, got[0]), (tag1, got[1])):
            want = single[tag, steps]
            assert same_bits(g[0], want[0]) and same_bits(g[1], want[1]), (tag0, tag1, steps, tag)
            assert g[2] == want[2], (tag0, tag1, steps, tag, g[2], want[2])
        return got

    for steps in (1, 2):
        check("a", a, "b", b, steps)
        check("b", b, "a", a, steps)
        check("a", a, "a", a, steps)
    # a system with xi = 0 at dx = dy = 0: its residual is 0, nothing can shrink, the first step is rejected -- and the other system goes on
    for steps in (1, 2):
        g0, g1 = check("zero", zero, "a", a, steps)
        assert g0[2]["rejected"] == 1 and g0[2]["accepted"] == 0 and not g0[0].any() and not g0[1].any()
        assert g1[2]["accepted"] >= 1
        g0, g1 = check("a", a, "zero", zero, steps)
        assert g1[2]["rejected"] == 1 and g1[2]["accepted"] == 0 and g0[2]["accepted"] >= 1
    kkt.close()


# ---- 6. new values -------------------------------------------------------------------------------------------------------------------
def test_k2_new_values_reach_the_copies_of_a():
    A, data = k2_input(*K2_INPUTS[0])
    th, rp, rd, xp, xd = data
    A2 = A.copy()
    A2.data = A.data * (1.0 + 0.25 * np.random.default_rng(8).standard_normal(A.nnz))
    kkt = handle(A, "K2")
    tk.update(kkt, th, rp, rd)
    dx0, dy0 = solved(kkt, xp, xd)
    polished(kkt, dx0, dy0, xp, xd, 1)                       # the copies of A are built here, from the old values
    nbytes = kkt.polish_report()["bytes"]
    tk.set_values(kkt, A2)
    tk.update(kkt, th, rp, rd)
    dx1, dy1 = solved(kkt, xp, xd)
    got = polished(kkt, dx1, dy1, xp, xd, 1)
    assert kkt.polish_report()["bytes"] == nbytes            # refreshed in place
    kkt.close()
    fresh = handle(A2, "K2")
    tk.update(fresh, th, rp, rd)
    fx, fy = solved(fresh, xp, xd)
    want = polished(fresh, fx, fy, xp, xd, 1)
    fresh.close()
    assert same_bits(dx1, fx) and same_bits(dy1, fy)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and got[2] == want[2]
    assert got[2]["accepted"] == 1


# ---- 7. the loops --------------------------------------------------------------------------------------------------------------------
def lpex():
    from ipm_harness import read_free_mps, standard_form
    return standard_form(read_free_mps(os.path.join(GOLDEN, "lpex_opt.mps")))


def run_loop(cls, d, **kw):
    return cls(d.A, d.b, d.c, d.l, d.u, c0=d.c0, objsense_min=d.objsense, device=0, **kw)


def final_point(opt):
    return [opt._get(k, opt.m if k in _lib.IPM_GET_ROWS else opt.n) for k in range(6)]


def loop_classes():
    from tulip_jl_amd.hsd_device import DeviceHSD
    from tulip_jl_amd.mpc_device import DeviceMPC
    return {"hsd": DeviceHSD, "mpc": DeviceMPC}


@pytest.mark.parametrize("loop", ["hsd", "mpc"])
def test_loops_with_polish_equal_the_loops_on_a_refine_handle(loop):
    cls, d = loop_classes()[loop], lpex()
    ref = run_loop(cls, d, refine=1).optimize()
    opt = run_loop(cls, d, polish=1).optimize()
    assert (opt.status, opt.niter) == (ref.status, ref.niter) and opt.status == "Trm_Optimal"
    for a, b in zip(final_point(opt), final_point(ref)):
        assert same_bits(a, b)
    assert opt.kkt.polish_report()["sides"][0]["asked"] == 1
    # polish = 0 after polish = 1 restores the plain run
    plain = run_loop(cls, d).optimize()
    opt.set_polish(0)
    opt.optimize()
    assert (opt.status, opt.niter) == (plain.status, plain.niter)
    for a, b in zip(final_point(opt), final_point(plain)):
        assert same_bits(a, b)


@pytest.mark.parametrize("loop", ["hsd", "mpc"])
def test_loops_on_k2_with_polish(loop):
    """Same status as the unpolished run, objectives within the loop's own tolerance (a relative gap of sqrt(eps)), accepted steps in the report.  The
    iteration counts are printed, not asserted: nobody has measured them."""
    cls, d = loop_classes()[loop], lpex()
    plain = run_loop(cls, d, system="K2").optimize()
    opt = run_loop(cls, d, system="K2", polish=1)
    accepted = 0
    step = opt.compute_step

    def counting_step(*a, **k):
        nonlocal accepted
        out = step(*a, **k)
        accepted += sum(s["accepted"] for s in opt.kkt.polish_report()["sides"])
        return out
    opt.compute_step = counting_step
    opt.optimize()
    print(f"{loop} K2: {plain.niter} iterations plain, {opt.niter} with polish=1; accepted steps seen at the end of the iterations: {accepted}")
    assert opt.status == plain.status == "Trm_Optimal"
    tol = float(np.sqrt(np.finfo(float).eps))
    assert abs(opt.primal_objective - plain.primal_objective) <= tol * (1 + abs(plain.primal_objective))
    assert abs(opt.dual_objective - plain.dual_objective) <= tol * (1 + abs(plain.dual_objective))
    assert opt.kkt.polish_report()["sides"][0]["asked"] == 1 and accepted > 0


# ---- 8. refusals that need a device --------------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    L = _lib.lib()
    A = random_lp_matrix(30, 50, 3, 3)
    th, rp, rd, xp, xd = ipm_like_data(30, 50, 0)
    bufs = [DevBuf(50), DevBuf(30), DevBuf(xp), DevBuf(xd)]
    ptrs = [b.ptr for b in bufs]
    for system in ("K1", "K2"):
        kkt = handle(A, system)
        assert L.tlpk_polish_device(kkt._h, *ptrs, 1) == _lib.NOT_FACTORED
        assert L.tlpk_polish2_device(kkt._h, *ptrs, *ptrs, 0) == _lib.NOT_FACTORED
        tk.update(kkt, th, rp, rd)
        kkt.solve_local(ptrs[2], ptrs[3])                                  # a pending split-phase solve
        assert L.tlpk_polish_device(kkt._h, *ptrs, 1) == _lib.BADARG
        assert L.tlpk_last_error(kkt._h).decode() == "tlpk_polish_device inside an unfinished split-phase solve, pair or refinement step"
        kkt.solve_finish(ptrs[0], ptrs[1], ptrs[3])
        kkt.sync()
        assert L.tlpk_polish_device(kkt._h, *ptrs, 1) == _lib.OK            # ... and the handle is as usable as before
        kkt.sync()
        assert L.tlpk_ipm_set_polish(kkt._h, 1) == _lib.BADARG and b"tlpk_ipm_load has not been called" in L.tlpk_last_error(kkt._h)
        kkt.close()
    from test_hsd_batch import load_batch, stacked_handle
    As, ro, co, vecs = stacked_handle()
    kkt = handle(As)
    rc, msg = load_batch(kkt, len(ro) - 1, ro, co, vecs)
    assert rc == _lib.OK, msg
    big = [DevBuf(As.shape[1]), DevBuf(As.shape[0]), DevBuf(As.shape[0], 1.0), DevBuf(As.shape[1], 1.0)]
    assert L.tlpk_polish_device(kkt._h, *[b.ptr for b in big], 1) == _lib.BADARG
    assert L.tlpk_last_error(kkt._h).decode() == "tlpk_polish_device: single-device handles with a factor only; this is a batch-loaded handle (tlpk_ipm_load_batch)"
    assert L.tlpk_ipm_set_polish(kkt._h, 1) == _lib.BADARG and b"a batch-loaded handle" in L.tlpk_last_error(kkt._h)
    kkt.close()


def test_first_use_allocation_is_held_against_the_budget():
    """A K2 handle whose budget leaves no room for the copies of A: TLPK_OOM from the first polish, nothing allocated, and the handle solves on."""
    A, data = k2_input(*K2_INPUTS[0])
    th, rp, rd, xp, xd = data
    free = handle(A, "K2")
    held = int(free.stats()["device_bytes"])
    tk.update(free, th, rp, rd)
    dx0, dy0 = solved(free, xp, xd)
    polished(free, dx0, dy0, xp, xd, 1)
    extra = free.polish_report()["bytes"]                           # what a first call allocates on this handle
    assert extra >= 16 * (A.shape[0] + A.shape[1]) + 24 * A.nnz and free.stats()["device_bytes"] == held + extra
    free.close()
    # the create-time gate works on an estimate: take the smallest budget it accepts among a few, starting just above what the handle really holds
    kkt = budget = None
    for budget in (held + 1024, held + extra // 2, held + extra - 8):
        try:
            kkt = handle(A, "K2", mem_budget_bytes=budget)
            break
        except tk.OutOfMemoryError:
            continue
    assert kkt is not None, "the create-time estimate exceeds what the handle and its first polish hold together: no budget can come between"
    assert kkt.stats()["device_bytes"] == held                      # nothing of the feature is allocated at create
    tk.update(kkt, th, rp, rd)
    dx0, dy0 = solved(kkt, xp, xd)
    bufs = [DevBuf(dx0), DevBuf(dy0), DevBuf(xp), DevBuf(xd)]
    assert _lib.lib().tlpk_polish_device(kkt._h, *[b.ptr for b in bufs], 1) == _lib.OOM
    assert "mem_budget_bytes" in _lib.lib().tlpk_last_error(kkt._h).decode()
    assert kkt.stats()["device_bytes"] == held and kkt.polish_report()["bytes"] == 0
    dx1, dy1 = solved(kkt, xp, xd)
    kkt.close()
    assert same_bits(dx1, dx0) and same_bits(dy1, dy0)
