"""Matrix-free K1 backend (tlpk_options.krylov = TLPK_KRYLOV_CG): conjugate gradients on (A D A' + Rd) dy = xi_p + A D xi_d on the device.

The comparator is `cg_restatement` below: the algorithm of include/tlpk.h / DESIGN.md section 1b'''' in numpy (Krylov.jl's stopping
rule: solved when sqrt(r' M^-1 r) <= atol + rtol sqrt(r0' M^-1 r0); tired after itmax = 2 m iterations; p' S p <= 0 ends it unsolved).
Every test that relies on convergence first asserts that the RESTATEMENT converges within half of itmax on its input, so that a bad
input fails as a bad input.  Inputs: the matrices of the table in DESIGN.md section 1b''''."""
import ctypes
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import tulip_jl_amd as tk
from tulip_jl_amd import _lib
from helpers import DevBuf, block_angular, ipm_like_data, kkt_residuals, random_lp_matrix

EPS = float(np.finfo(np.float64).eps)
SQRT_EPS = float(np.sqrt(EPS))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def _fixture_2x4():
    return sp.csc_matrix(np.array([[1.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 1.0]]))          # test/KKT/Krylov/spd.jl


def _long_row_col():
    """600 x 1500, seed 2: one full row, one full column, one empty row, one empty column -- the long and the short kind of row and
    column in one launch."""
    rng = np.random.default_rng(2)
    A = random_lp_matrix(600, 1500, 4, 2).tolil()
    A[7, :] = rng.standard_normal(1500)          # full row
    A[:, 11] = rng.standard_normal((600, 1))     # full column
    A[300, :] = 0.0                              # empty row
    A[:, 700] = 0.0                              # empty column
    A = A.tocsc(); A.eliminate_zeros(); A.sort_indices()
    return A


MATRICES = {
    "fixture": _fixture_2x4,
    "r1x5": lambda: random_lp_matrix(1, 5, 1, 1),
    "r40x10": lambda: random_lp_matrix(40, 10, 3, 1),
    "r30x50": lambda: random_lp_matrix(30, 50, 3, 1),
    "r500": lambda: random_lp_matrix(500, 1200, 4, 1),
    "r3000": lambda: random_lp_matrix(3000, 7000, 4, 1),
    "long600": _long_row_col,
    "ba1220": lambda: block_angular(4, 300, 600, 20, 3, 0.3, 5)[0],
}
# the first ten rows of the table: (matrix, regime, converges without a preconditioner)
ROWS = [("fixture", "unit", True), ("r1x5", "unit", True), ("r40x10", "unit", True), ("r30x50", "unit", True), ("r500", "unit", True),
        ("r500", "mid", False), ("r3000", "unit", True), ("r3000", "mid", False), ("long600", "unit", True), ("ba1220", "unit", True)]
CONVERGING = [(mat, reg, pre) for mat, reg, ok in ROWS for pre in (None, "jacobi") if ok or pre == "jacobi"]
IDS = [f"{mat}-{reg}-{pre or 'none'}" for mat, reg, pre in CONVERGING]


@functools.lru_cache(maxsize=None)
def matrix(name):
    A = sp.csc_matrix(MATRICES[name]())
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def data(name, regime):
    A = matrix(name)
    m, n = A.shape
    if name == "fixture":
        return tuple(np.ones(k) for k in (n, n, m, m, n))
    return ipm_like_data(m, n, 1, regime)


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def cg_restatement(A, th, rp, rd, xp, xd, precond=None, itmax=0, atol=0.0, rtol=0.0):
    """-> dict(dy, dx, iters, converged, resid0, resid)"""
    A = sp.csr_matrix(A)
    m, n = A.shape
    At = A.T.tocsr()
    D = 1.0 / (th + rp)
    itmax = itmax or 2 * m
    atol = atol or SQRT_EPS; rtol = rtol or SQRT_EPS
    Minv = 1.0 / (A.multiply(A) @ D + rd) if precond == "jacobi" else np.ones(m)
    b = xp + A @ (D * xd)
    x = np.zeros(m); r = b.copy(); z = Minv * r; p = z.copy()
    gamma = float(r @ z)
    rho0 = rho = np.sqrt(gamma)
    tol = atol + rtol * rho0
    k = 0
    solved = rho <= tol
    while not solved and k < itmax:
        q = A @ (D * (At @ p)) + rd * p
        pq = float(p @ q)
        if not (pq > 0.0) or not np.isfinite(pq):
            break
        alpha = gamma / pq
        x += alpha * p; r -= alpha * q
        z = Minv * r
        g1 = float(r @ z)
        k += 1
        rho = np.sqrt(g1)
        solved = rho <= tol
        p = z + (g1 / gamma) * p
        gamma = g1
    dx = D * (At @ x - xd)
    return dict(dy=x, dx=dx, iters=k, converged=bool(solved), resid0=float(rho0), resid=float(rho), itmax=itmax)


@functools.lru_cache(maxsize=None)
def restated(name, regime, precond):
    A = matrix(name)
    out = cg_restatement(A, *data(name, regime), precond=precond)
    return out


@functools.lru_cache(maxsize=None)
def dense_reference(name, regime):
    """S (sparse), b, dy* = S \\ b (LAPACK), lambda_min(S), the diagonal of S"""
    A = matrix(name)
    th, rp, rd, xp, xd = data(name, regime)
    D = 1.0 / (th + rp)
    S = (A @ sp.diags(D) @ A.T + sp.diags(rd)).tocsr()
    Sd = S.toarray()
    b = xp + A @ (D * xd)
    return S, b, np.linalg.solve(Sd, b), float(np.linalg.eigvalsh(Sd)[0]), Sd.diagonal().copy()


def assert_good_input(name, regime, precond):
    ref = restated(name, regime, precond)
    assert ref["converged"] and ref["iters"] <= ref["itmax"] // 2, f"bad test input {name}/{regime}/{precond}: the restatement needs {ref['iters']} of {ref['itmax']}"
    return ref


def krylov(A, device=0, **kw):
    return tk.setup(A, tk.K1(), tk.KrylovBackend(device=device, **kw))


def solve_on(kkt, th, rp, rd, xp, xd):
    tk.update(kkt, th, rp, rd)
    dx = np.zeros(kkt.n); dy = np.zeros(kkt.m)
    tk.solve(dx, dy, kkt, xp, xd)
    return dx, dy


@functools.lru_cache(maxsize=None)
def device_solution(name, regime, precond):
    """one solve on the device per table row, shared by the tests that look at it: (dx, dy, stats)"""
    kkt = krylov(matrix(name), precond=precond)
    dx, dy = solve_on(kkt, *data(name, regime))
    st = kkt.stats()
    kkt.close()
    return dx, dy, st


def gap_bound(name, regime, precond, dy, k):
    """g = 4 k eps (|S|inf |dy|inf + |b|inf) sqrt(m max_i M^-1_i): the standard bound on the distance between the recurrence residual
    and the true one after k steps, in the M^-1 norm"""
    S, b, _, _, diag = dense_reference(name, regime)
    m = S.shape[0]
    Minv = 1.0 / diag if precond == "jacobi" else np.ones(m)
    s_inf = float(abs(S).sum(axis=1).max())
    return 4.0 * k * EPS * (s_inf * np.abs(dy).max(initial=0.0) + np.abs(b).max(initial=0.0)) * np.sqrt(m * Minv.max()), Minv


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _raw_create(A, fn="tlpk_create", **fields):
    L = _lib.lib()
    A = sp.csc_matrix(A); A.sort_indices()
    m, n = A.shape
    opt = _lib.Options(); L.tlpk_default_options(ctypes.byref(opt))
    opt.device = -1
    opt.krylov = _lib.KRYLOV_CG
    keep = []
    for k, v in fields.items():
        if isinstance(v, np.ndarray):
            keep.append(v); v = _lib.as_p64(v)
        setattr(opt, k, v)
    h = ctypes.c_void_p()
    colptr = A.indptr.astype(np.int64); rowval = A.indices.astype(np.int64); nz = np.ascontiguousarray(A.data, dtype=np.float64)
    if fn == "tlpk_create":
        rc = L.tlpk_create(ctypes.byref(h), m, n, _lib.as_p64(colptr), _lib.as_p64(rowval), _lib.as_pd(nz), 0, ctypes.byref(opt))
    elif fn == "tlpk_create_multi":
        rc = L.tlpk_create_multi(ctypes.byref(h), m, n, _lib.as_p64(colptr), _lib.as_p64(rowval), _lib.as_pd(nz), 0, ctypes.byref(opt), 2, None)
    else:
        Ad = np.asfortranarray(A.toarray())
        rc = L.tlpk_create_dense(ctypes.byref(h), m, n, Ad.ctypes.data_as(_lib.pd), m, ctypes.byref(opt))
    return rc, h, L.tlpk_last_create_error().decode()


def test_defaults_and_struct_size():
    opt = _lib.Options()
    _lib.lib().tlpk_default_options(ctypes.byref(opt))
    assert opt.struct_size == ctypes.sizeof(_lib.Options)
    assert opt.krylov == 0 and opt.krylov_precond == 0 and opt.krylov_itmax == 0 and opt.krylov_atol == 0.0 and opt.krylov_rtol == 0.0
    assert _lib.KRYLOV_CG == 1


@pytest.mark.parametrize("name", ["fixture", "r30x50", "r3000"])
def test_analyse_only_handle_has_no_symbolic_structure(name):
    A = matrix(name)
    kkt = krylov(A, device=-1)
    st = kkt.stats()
    assert (st["m"], st["n"], st["nnzA"]) == (A.shape[0], A.shape[1], A.nnz)
    for key in ("nnzS", "nnzL", "nnzL_stored", "n_pairs", "n_supernodes", "flops_chol", "flops_panel", "flops_update", "flops_update_alg", "flops_syrk"):
        assert st[key] == 0, key
    assert (kkt.perm() == np.arange(A.shape[0])).all()
    for what in ("s_colptr", "s_rowidx", "etree", "colcount", "rowidx", "pair_ptr", "factor_launches", "fwd_launches", "bwd_launches", "front_f"):
        arr = kkt.symbolic(what)
        assert arr.size == 0 or (what == "pair_ptr" and arr.tolist() == [0]), what
    for key in ("krylov_iters", "krylov_iters_total", "krylov_converged", "krylov_resid0", "krylov_resid"):
        assert st[key] == 0


@pytest.mark.parametrize("fields", [
    dict(system=_lib.SYSTEM_K2), dict(nranks=2), dict(dense_cols=1), dict(refine_steps=1), dict(user_perm=np.arange(30, dtype=np.int64)),
    dict(krylov=2), dict(krylov=-1), dict(krylov_precond=2), dict(krylov_precond=-1), dict(krylov_itmax=-1),
    dict(krylov_atol=-1.0), dict(krylov_rtol=float("nan")), dict(krylov_atol=float("inf")),
], ids=lambda f: ",".join(f"{k}" if isinstance(v, np.ndarray) else f"{k}={v}" for k, v in f.items()))
def test_create_refuses(fields):
    rc, h, msg = _raw_create(matrix("r30x50"), **fields)
    assert rc == _lib.BADARG and not h and msg


def test_create_multi_and_create_dense_refuse():
    A, rb = block_angular(4, 20, 40, 6, 3, 0.5, 2)
    rc, h, msg = _raw_create(A, "tlpk_create_multi", row_block=np.ascontiguousarray(rb, dtype=np.int64))
    assert rc == _lib.BADARG and not h and "krylov" in msg
    rc, h, msg = _raw_create(matrix("r30x50"), "tlpk_create_dense")
    assert rc == _lib.BADARG and not h and "krylov" in msg
    with pytest.raises(TypeError):
        tk.setup(matrix("r30x50"), tk.K2(), tk.KrylovBackend(device=-1))
    with pytest.raises(ValueError):
        tk.KrylovBackend(precond="ilu")


def test_device_loops_take_the_backend_with_its_own_fields_only():
    from tulip_jl_amd.hsd_device import DeviceHSD
    A = matrix("r30x50")
    m, n = A.shape
    args = (A, np.ones(m), np.ones(n), np.zeros(n), np.full(n, np.inf))
    with pytest.raises(TypeError):
        DeviceHSD(*args, backend=tk.KrylovBackend(device=-1), streams=2)          # an option of the direct backend
    with pytest.raises(TypeError):
        DeviceHSD(*args, backend=tk.Backend(device=-1))
    with pytest.raises(TypeError):
        DeviceHSD(*args, backend=tk.KrylovBackend(device=-1), dense=True)


def test_ignored_options_do_not_refuse():
    rb = np.zeros(30, dtype=np.int64)
    rc, h, _ = _raw_create(matrix("r30x50"), row_block=rb, detect_blocks=1, ordering=_lib.ORDER_NATURAL, relax=0, streams=3)
    assert rc == _lib.OK and h
    _lib.lib().tlpk_destroy(h)


def test_memory_gate_counts_a_and_the_vectors():
    A = matrix("r3000")
    with pytest.raises(tk.OutOfMemoryError) as e:
        krylov(A, device=-1, mem_budget_bytes=100000)
    assert "bytes" in str(e.value)
    krylov(A, device=-1, mem_budget_bytes=36 * A.nnz + 80 * A.shape[1] + 136 * A.shape[0] + 65536).close()


def test_numeric_calls_need_a_device_and_there_is_no_factor():
    A = matrix("r30x50")
    kkt = krylov(A, device=-1)
    L = _lib.lib()
    th, rp, rd, xp, xd = data("r30x50", "unit")
    assert L.tlpk_update(kkt._h, _lib.as_pd(th), _lib.as_pd(rp), _lib.as_pd(rd)) == _lib.NO_DEVICE
    buf = np.zeros(8)
    assert L.tlpk_get_factor(kkt._h, _lib.as_pd(buf), 8) == _lib.BADARG and b"no factor" in L.tlpk_last_error(kkt._h)
    p = ctypes.c_void_p(); cnt = ctypes.c_int64()
    calls = [("tlpk_update_local", (None, None, None)), ("tlpk_update_finish", ()), ("tlpk_solve_local", (None, None)),
             ("tlpk_solve_finish", (None, None, None)), ("tlpk_solve2_local", (None,) * 4), ("tlpk_solve2_finish", (None,) * 6),
             ("tlpk_refine_local", (None,) * 4), ("tlpk_refine_finish", (None, None)), ("tlpk_root_copy", (0, 0, None)),
             ("tlpk_root_panel", (ctypes.byref(p), ctypes.byref(cnt))), ("tlpk_root_rhs", (ctypes.byref(p), ctypes.byref(cnt))),
             ("tlpk_root_rhs2", (ctypes.byref(p), ctypes.byref(cnt)))]
    for name, args in calls:
        assert getattr(L, name)(kkt._h, *args) == _lib.BADARG, name
        assert b"matrix-free" in L.tlpk_last_error(kkt._h), name


def test_backend_text():
    A = matrix("r30x50")
    assert tk.backend(krylov(A, device=-1)) == "HIP (gfx950) CG"
    assert tk.backend(krylov(A, device=-1, precond="jacobi")).startswith("HIP (gfx950) CG")
    assert tk.backend(tk.setup(A, tk.K1(), tk.Backend(device=-1))) == "HIP (gfx950)"
    assert tk.linear_system(krylov(A, device=-1)) == "Normal equations (K1)"


def test_direct_handle_reports_zero_krylov_stats():
    st = tk.setup(matrix("r30x50"), tk.K1(), tk.Backend(device=-1)).stats()
    for key in ("krylov_iters", "krylov_iters_total", "krylov_converged", "krylov_resid0", "krylov_resid"):
        assert st[key] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reference_conformance_fixture():
    A = matrix("fixture")
    for pre in (None, "jacobi"):
        kkt = krylov(A, precond=pre)
        tk.run_ls_tests(A, kkt)
        st = kkt.stats()
        assert st["krylov_iters"] == 1 and st["krylov_converged"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("mat,reg,pre", CONVERGING, ids=IDS)
def test_stopping_rule_is_honoured(mat, reg, pre):
    assert_good_input(mat, reg, pre)
    _, dy, st = device_solution(mat, reg, pre)
    S, b, _, _, _ = dense_reference(mat, reg)
    g, Minv = gap_bound(mat, reg, pre, dy, st["krylov_iters"])
    r = b - S @ dy
    rho = float(np.sqrt(r @ (Minv * r))); rho0 = float(np.sqrt(b @ (Minv * b)))
    tol = SQRT_EPS + SQRT_EPS * rho0
    print(f"{mat}/{reg}/{pre}: k={st['krylov_iters']} true rho={rho:.3e} recurrence rho={st['krylov_resid']:.3e} tol={tol:.3e} gap={abs(rho - st['krylov_resid']):.3e} g={g:.3e}")
    assert st["krylov_converged"] == 1
    assert rho <= tol + g
    assert abs(st["krylov_resid0"] - rho0) <= 1e-12 * rho0 + 1e-300


@pytest.mark.gpu
@pytest.mark.parametrize("mat,reg,pre", CONVERGING, ids=IDS)
def test_solution(mat, reg, pre):
    assert_good_input(mat, reg, pre)
    dx, dy, st = device_solution(mat, reg, pre)
    A = matrix(mat)
    th, rp, rd, xp, xd = data(mat, reg)
    S, b, dy_star, lam_min, diag = dense_reference(mat, reg)
    g, Minv = gap_bound(mat, reg, pre, dy, st["krylov_iters"])
    rho0 = float(np.sqrt(b @ (Minv * b)))
    bound = ((SQRT_EPS + SQRT_EPS * rho0) + g) * np.sqrt((1.0 / Minv).max()) / lam_min
    err = float(np.linalg.norm(dy - dy_star))
    _, r2 = kkt_residuals(A, th, rp, rd, xp, xd, dx, dy)
    a_inf = float(abs(A).sum(axis=1).max())
    r2_bound = 100 * EPS * (np.abs(dx).max() * (th + rp).max() + a_inf * np.abs(dy).max() + np.abs(xd).max())
    print(f"{mat}/{reg}/{pre}: |dy - dy*|2={err:.3e} bound={bound:.3e}  r2={r2:.3e} bound={r2_bound:.3e}")
    assert err <= bound
    assert r2 <= r2_bound


@pytest.mark.gpu
@pytest.mark.parametrize("mat,reg,pre", CONVERGING, ids=IDS)
def test_iteration_count(mat, reg, pre):
    ref = assert_good_input(mat, reg, pre)
    _, _, st = device_solution(mat, reg, pre)
    print(f"{mat}/{reg}/{pre}: device {st['krylov_iters']} iterations, restatement {ref['iters']} (itmax {ref['itmax']})")
    assert 0 <= st["krylov_iters"] <= ref["itmax"]
    assert st["krylov_iters"] == st["krylov_iters_total"]


@pytest.mark.gpu
def test_not_converged_is_reported_not_hidden():
    ref = restated("r500", "mid", None)
    assert not ref["converged"] and ref["iters"] == 1000            # the input guard of this test: the restatement stalls too
    A = matrix("r500")
    kkt = krylov(A)
    dx, dy = solve_on(kkt, *data("r500", "mid"))                    # returns: TLPK_OK
    st = kkt.stats()
    assert st["krylov_converged"] == 0 and st["krylov_iters"] == 1000 == 2 * A.shape[0]
    assert np.isfinite(dx).all() and np.isfinite(dy).all()
    assert kkt.symbolic("krylov_unsolved")[0] == 1
    # the same handle, new update, data it can solve
    assert_good_input("r500", "unit", None)
    dx, dy = solve_on(kkt, *data("r500", "unit"))
    st = kkt.stats()
    assert st["krylov_converged"] == 1 and st["krylov_iters"] == st["krylov_iters_total"]
    _, _, dy_star, _, _ = dense_reference("r500", "unit")
    assert np.linalg.norm(dy - dy_star) <= 1e-6 * np.linalg.norm(dy_star)
    # itmax is honoured exactly
    k5 = krylov(A, itmax=5)
    solve_on(k5, *data("r500", "unit"))
    st = k5.stats()
    assert st["krylov_iters"] == 5 and st["krylov_converged"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("pre", [None, "jacobi"])
def test_bitwise_contracts(pre):
    A = matrix("long600")
    m, n = A.shape
    th, rp, rd, xp, xd = data("long600", "unit")
    assert_good_input("long600", "unit", pre)
    kkt = krylov(A, precond=pre)
    # a solve before any update
    assert _lib.lib().tlpk_solve(kkt._h, _lib.as_pd(np.zeros(n)), _lib.as_pd(np.zeros(m)), _lib.as_pd(xp), _lib.as_pd(xd)) == _lib.NOT_FACTORED
    dx0, dy0 = solve_on(kkt, th, rp, rd, xp, xd)
    it0 = kkt.stats()["krylov_iters"]
    dx1 = np.zeros(n); dy1 = np.zeros(m)
    tk.solve(dx1, dy1, kkt, xp, xd)
    assert (dx0 == dx1).all() and (dy0 == dy1).all()                # two solves of the same data
    assert kkt.stats()["krylov_iters_total"] == 2 * it0
    # device pointers
    b_xp, b_xd, b_dx, b_dy = DevBuf(xp), DevBuf(xd), DevBuf(n), DevBuf(m)
    kkt.solve_device(b_dx.ptr, b_dy.ptr, b_xp.ptr, b_xd.ptr)
    assert (b_dx.get() == dx0).all() and (b_dy.get() == dy0).all()
    # a pair = two solves
    xp2, xd2 = np.cos(np.arange(m)), np.sin(np.arange(n))
    dx2 = np.zeros(n); dy2 = np.zeros(m)
    tk.solve(dx2, dy2, kkt, xp2, xd2)
    c_xp, c_xd, c_dx, c_dy = DevBuf(xp2), DevBuf(xd2), DevBuf(n), DevBuf(m)
    kkt.solve2_device(b_dx.ptr, b_dy.ptr, b_xp.ptr, b_xd.ptr, c_dx.ptr, c_dy.ptr, c_xp.ptr, c_xd.ptr)
    assert (b_dx.get() == dx0).all() and (b_dy.get() == dy0).all() and (c_dx.get() == dx2).all() and (c_dy.get() == dy2).all()
    # a zero right-hand side
    dxz = np.ones(n); dyz = np.ones(m)
    tk.solve(dxz, dyz, kkt, np.zeros(m), np.zeros(n))
    st = kkt.stats()
    assert not dxz.any() and not dyz.any() and st["krylov_iters"] == 0 and st["krylov_converged"] == 1
    # update / solve / update / solve against fresh handles
    th2 = th * 1.7 + 0.1
    dx3, dy3 = solve_on(kkt, th2, rp, rd, xp, xd)
    dx4, dy4 = solve_on(kkt, th, rp, rd, xp, xd)
    f1, f2 = krylov(A, precond=pre), krylov(A, precond=pre)
    fx3, fy3 = solve_on(f1, th2, rp, rd, xp, xd)
    fx4, fy4 = solve_on(f2, th, rp, rd, xp, xd)
    assert (dx3 == fx3).all() and (dy3 == fy3).all() and (dx4 == fx4).all() and (dy4 == fy4).all()
    assert (dx4 == dx0).all() and (dy4 == dy0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("pre", [None, "jacobi"])
def test_set_values_equals_a_fresh_handle(pre):
    A = matrix("r500")
    th, rp, rd, xp, xd = data("r500", "unit")
    B = A.copy(); B.data = A.data * np.linspace(0.5, 1.5, A.nnz)
    assert cg_restatement(B, th, rp, rd, xp, xd, precond=pre)["iters"] <= A.shape[0]          # input guard (half of itmax = m)
    kkt = krylov(A, precond=pre)
    solve_on(kkt, th, rp, rd, xp, xd)
    tk.set_values(kkt, B)
    assert _lib.lib().tlpk_solve(kkt._h, _lib.as_pd(np.zeros(A.shape[1])), _lib.as_pd(np.zeros(A.shape[0])), _lib.as_pd(xp), _lib.as_pd(xd)) == _lib.NOT_FACTORED
    dx, dy = solve_on(kkt, th, rp, rd, xp, xd)
    fx, fy = solve_on(krylov(B, precond=pre), th, rp, rd, xp, xd)
    assert (dx == fx).all() and (dy == fy).all()
    assert kkt.stats()["krylov_converged"] == 1


HSD_STATUS = {"lpex_opt": "Trm_Optimal", "lpex_freevars": "Trm_Optimal", "lpex_inf": "Trm_PrimalInfeasible", "lpex_ubd": "Trm_DualInfeasible"}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HSD_STATUS))
def test_device_resident_hsd(name):
    from tulip_jl_amd.hsd_device import DeviceHSD
    from tulip_jl_amd.problem import read_free_mps, standard_form
    d = standard_form(read_free_mps(os.path.join(GOLDEN, name + ".mps")))
    direct = DeviceHSD(d.A, d.b, d.c, d.l, d.u, c0=d.c0, objsense_min=d.objsense, device=0).optimize()
    assert direct.status == HSD_STATUS[name]
    for pre in (None, "jacobi"):
        opt = DeviceHSD(d.A, d.b, d.c, d.l, d.u, c0=d.c0, objsense_min=d.objsense, backend=tk.KrylovBackend(precond=pre)).optimize()
        print(f"{name}/{pre}: {opt.status} in {opt.niter} iterations, z = {opt.primal_objective!r} (direct {direct.primal_objective!r}), {opt.timers['n_solve']} solves")
        assert opt.status == HSD_STATUS[name]
        if opt.status == "Trm_Optimal":
            assert abs(opt.primal_objective - direct.primal_objective) <= 1e-6 * (1 + abs(direct.primal_objective))
        assert opt.kkt.symbolic("krylov_unsolved")[0] == 0              # every solve met the stopping rule
        assert opt.timers["n_solve"] > 0


@pytest.mark.gpu
def test_profile_mode_times_the_solve_as_spmv():
    A = matrix("r500")
    assert_good_input("r500", "unit", "jacobi")
    kkt = krylov(A, precond="jacobi", profile=True)
    solve_on(kkt, *data("r500", "unit"))
    kt, st = kkt.kernel_times(), kkt.stats()
    assert kt["spmv"]["launches"] >= 3 and kt["spmv"]["ms"] > 0.0            # right-hand side + set-up, at least one chunk, dy / dx
    for cls in ("extend_add", "potrf", "trsm", "update", "solve_fwd", "solve_bwd", "update_reduce", "chain"):
        assert kt[cls]["launches"] == 0, cls
    assert st["ms_last_solve"] >= kt["spmv"]["ms"] * 0.5 and st["krylov_converged"] == 1
    assert st["launches_update"] == 2 and st["launches_solve"] >= 5 + 4 * st["krylov_iters"]


class _RestatementBackend:
    """cg_restatement behind the three calls tests/ipm_harness.py asks of a KKT backend"""

    def __init__(self, A):
        self.A, self.unsolved = A, 0

    def update(self, th, rp, rd):
        self.args = (th.copy(), rp.copy(), rd.copy())

    def solve(self, dx, dy, xp, xd):
        out = cg_restatement(self.A, *self.args, xp, xd)
        dx[:] = out["dx"]; dy[:] = out["dy"]
        self.unsolved += not out["converged"]


@pytest.mark.gpu
def test_device_resident_mpc_accepts_the_backend():
    """DeviceMPC runs through the same solve path.  No preconditioner: with Jacobi the restatement itself ends this LP in Trm_IterationLimit at
    z = 1.50017 (DESIGN.md section 1b'''', limits), so that combination is no test input."""
    from ipm_harness import read_free_mps as read_ref, solve_lp
    from tulip_jl_amd.mpc_device import DeviceMPC
    from tulip_jl_amd.problem import read_free_mps, standard_form
    path = os.path.join(GOLDEN, "lpex_opt.mps")
    made = []
    ref, _ = solve_lp(read_ref(path), lambda A: made.append(_RestatementBackend(A)) or made[-1], algorithm="mpc")
    assert ref.status == "Trm_Optimal" and made[0].unsolved == 0, "bad test input: the restatement does not solve it"
    d = standard_form(read_free_mps(path))
    direct = DeviceMPC(d.A, d.b, d.c, d.l, d.u, c0=d.c0, objsense_min=d.objsense, device=0).optimize()
    opt = DeviceMPC(d.A, d.b, d.c, d.l, d.u, c0=d.c0, objsense_min=d.objsense, backend=tk.KrylovBackend()).optimize()
    print(f"MPC lpex_opt: {opt.status} in {opt.niter} iterations, z = {opt.primal_objective!r} (direct {direct.status}, {direct.primal_objective!r})")
    assert opt.status == direct.status == "Trm_Optimal"
    assert abs(opt.primal_objective - direct.primal_objective) <= 1e-6 * (1 + abs(direct.primal_objective))
    assert opt.kkt.symbolic("krylov_unsolved")[0] == 0
    with pytest.raises(TypeError):
        DeviceMPC(d.A, d.b, d.c, d.l, d.u, system="K2", backend=tk.KrylovBackend())


@pytest.mark.gpu
def test_device_beside_the_backend_object_overrides_its_field():
    """Model(..., backend=KrylovBackend(), device=0): device, profile and mem_budget_bytes are fields of the backend object too"""
    from tulip_jl_amd.hsd_device import DeviceHSD
    from tulip_jl_amd.problem import read_free_mps, standard_form
    d = standard_form(read_free_mps(os.path.join(GOLDEN, "lpex_opt.mps")))
    be = tk.KrylovBackend(device=-1)
    opt = DeviceHSD(d.A, d.b, d.c, d.l, d.u, c0=d.c0, objsense_min=d.objsense, backend=be, device=0)
    assert be.device == -1 and opt.kkt.backend_options.device == 0               # a copy: the caller's object is not changed
    assert opt.optimize().status == "Trm_Optimal"
