"""Matrix-free K2 backend in its quasi-definite form (tlpk_options.krylov = TLPK_KRYLOV_TRICG): TriCG on [Rd A; A' -E] [dy; dx] = [xi_p; xi_d] on the device.

The comparator is `tricg_restatement` below: the algorithm of include/tlpk.h / DESIGN.md section 1b'''''' in numpy (two short recurrences that
tridiagonalise A in the Rd and E inner products, the 2 x 2 block L D L' of the permuted projected matrix; solved when
rho_k <= atol + rtol rho_0; tired after itmax = 2 (m + n) iterations; a pivot block that loses its signature ends it unsolved).  Every test that
relies on convergence first asserts that the RESTATEMENT converges within half of itmax on its input.  Inputs: the matrices of the table of
tests/test_krylov_k2.py.  Vectors of order n + m are ordered [dx; dy] as a K2 handle numbers its nodes, K = [-E A'; A Rd], W = diag(E, Rd).

Restatement iteration counts: fixture 1, r1x5 2, r40x10 25, r30x50 30, r500 68, long600 86, ba1220 80 (all "unit"), r30x50 "mid" 67 of 160;
r40x10 "mid" stops at itmax = 100 unsolved."""
import ctypes
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import tulip_jl_amd as tk
from tulip_jl_amd import _lib
from helpers import DevBuf, block_angular, ipm_like_data, random_lp_matrix

KRYLOV = _lib.KRYLOV_TRICG          # (without the method this module does not import: none of its tests can pass)
EPS = float(np.finfo(np.float64).eps)
SQRT_EPS = float(np.sqrt(EPS))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs (the constructions of tests/test_krylov_k2.py's table)
# ---------------------------------------------------------------------------------------------------------------------------------
def _long_row_col():
    """600 x 1500, seed 2: one full row, one full column, one empty row, one empty column"""
    rng = np.random.default_rng(2)
    A = random_lp_matrix(600, 1500, 4, 2).tolil()
    A[7, :] = rng.standard_normal(1500)
    A[:, 11] = rng.standard_normal((600, 1))
    A[300, :] = 0.0
    A[:, 700] = 0.0
    A = A.tocsc(); A.eliminate_zeros(); A.sort_indices()
    return A


MATRICES = {
    "fixture": lambda: sp.csc_matrix(np.array([[1.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 1.0]])),
    "r1x5": lambda: random_lp_matrix(1, 5, 1, 1),
    "r40x10": lambda: random_lp_matrix(40, 10, 3, 1),
    "r30x50": lambda: random_lp_matrix(30, 50, 3, 1),
    "r500": lambda: random_lp_matrix(500, 1200, 4, 1),
    "long600": _long_row_col,
    "ba1220": lambda: block_angular(4, 300, 600, 20, 3, 0.3, 5)[0],
}
# (matrix, regime) of every row that converges, and the restatement's iteration count
CONVERGING = [(mat, "unit") for mat in ("fixture", "r1x5", "r40x10", "r30x50", "r500", "long600", "ba1220")] + [("r30x50", "mid")]
COUNTS = [1, 2, 25, 30, 68, 86, 80, 67]
IDS = [f"{mat}-{reg}" for mat, reg in CONVERGING]


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
def _scaled(w, norm):
    return w / norm if norm > 0.0 else np.zeros_like(w)


def tricg_restatement(A, th, rp, rd, xp, xd, itmax=0, atol=0.0, rtol=0.0):
    """-> dict(dx, dy, x = [dx; dy], iters, converged, resid0, resid, itmax)"""
    A = sp.csr_matrix(A)
    m, n = A.shape
    At = A.T.tocsr()
    E = th + rp
    itmax = itmax or 2 * (m + n)
    atol = atol or SQRT_EPS; rtol = rtol or SQRT_EPS
    q = np.array(xp, dtype=float); p = np.array(xd, dtype=float)
    beta = beta1 = float(np.sqrt(q @ (q / rd))); gamma = gamma1 = float(np.sqrt(p @ (p / E)))
    rho = rho0 = float(np.hypot(beta1, gamma1)); tol = atol + rtol * rho0
    solved = rho0 <= tol
    v = _scaled(q / rd, beta1); u = _scaled(p / E, gamma1)
    v_old = np.zeros(m); u_old = np.zeros(n)
    dy = np.zeros(m); dx = np.zeros(n)
    Gx = np.zeros((m, 2)); Gy = np.zeros((n, 2))
    Dinv = np.zeros((2, 2)); pi = np.zeros(2)
    k = 0
    while not solved and k < itmax:
        k += 1
        q = A @ u - gamma * (rd * v_old); p = At @ v - beta * (E * u_old)
        alpha = float(v @ q)
        q = q - alpha * (rd * v); p = p - alpha * (E * u)
        Omega = np.array([[1.0, alpha], [alpha, -1.0]])
        if k == 1:
            Lam = np.zeros((2, 2)); D = Omega; g = np.array([beta1, gamma1])
        else:
            Psi = np.array([[0.0, beta], [gamma, 0.0]])
            Lam = Psi @ Dinv; D = Omega - Lam @ Psi.T; g = -Psi @ pi
        det = float(D[0, 0] * D[1, 1] - D[0, 1] * D[1, 0])
        if not (det < 0.0) or not np.isfinite(det):
            break
        Dinv = np.array([[D[1, 1], -D[0, 1]], [-D[1, 0], D[0, 0]]]) / det
        pi = Dinv @ g
        Gx = np.column_stack([v, np.zeros(m)]) - Gx @ Lam.T
        Gy = np.column_stack([np.zeros(n), u]) - Gy @ Lam.T
        dy = dy + Gx @ pi; dx = dx + Gy @ pi
        beta = float(np.sqrt(q @ (q / rd))); gamma = float(np.sqrt(p @ (p / E)))
        v_old, u_old = v, u
        v = _scaled(q / rd, beta); u = _scaled(p / E, gamma)
        rho = float(np.hypot(beta * pi[1], gamma * pi[0]))
        if not np.isfinite(rho):
            break
        solved = rho <= tol
    return dict(dx=dx, dy=dy, x=np.concatenate([dx, dy]), iters=k, converged=bool(solved), resid0=rho0, resid=rho, itmax=itmax)


@functools.lru_cache(maxsize=None)
def restated(name, regime):
    return tricg_restatement(matrix(name), *data(name, regime))


def _dense(A, th, rp, rd, xp, xd):
    E = th + rp
    K = sp.bmat([[-sp.diags(E), A.T], [A, sp.diags(rd)]]).tocsr()
    Kd = K.toarray()
    b = np.concatenate([xd, xp])
    return K, b, np.linalg.solve(Kd, b), float(np.abs(np.linalg.eigvalsh(Kd)).min()), np.concatenate([E, rd])


@functools.lru_cache(maxsize=None)
def dense_reference(name, regime):
    """K (sparse), b, x* = K \\ b (LAPACK), sigma_min(K), W = diag(E, Rd)"""
    return _dense(matrix(name), *data(name, regime))


def assert_good_input(name, regime):
    ref = restated(name, regime)
    assert ref["converged"] and ref["iters"] <= ref["itmax"] // 2, f"bad test input {name}/{regime}: the restatement needs {ref['iters']} of {ref['itmax']}"
    return ref


def _gap(dense, x, k):
    """g = 4 k eps (|K|inf |x|inf + |b|inf) sqrt(N max_i W^-1_i): tests/test_krylov_k2.py's gap_bound with M^-1 = W^-1"""
    K, b, _, _, W = dense
    N = K.shape[0]
    k_inf = float(abs(K).sum(axis=1).max())
    return 4.0 * k * EPS * (k_inf * np.abs(x).max(initial=0.0) + np.abs(b).max(initial=0.0)) * np.sqrt(N * (1.0 / W).max())


def _check(dense, x, k, what):
    """|x - x*|2 <= (tol + g) sqrt(max W) / sigma_min(K)"""
    _, b, x_star, sig_min, W = dense
    g = _gap(dense, x, k)
    rho0 = float(np.sqrt(b @ (b / W)))
    bound = ((SQRT_EPS + SQRT_EPS * rho0) + g) * np.sqrt(W.max()) / sig_min
    err = float(np.linalg.norm(x - x_star))
    print(f"{what}: k={k} |x - x*|2={err:.3e} bound={bound:.3e} (g={g:.3e}, sigma_min={sig_min:.3e})")
    assert err <= bound


def gap_bound(name, regime, x, k):
    return _gap(dense_reference(name, regime), x, k)


def check_solution(name, regime, x, k, what):
    _check(dense_reference(name, regime), x, k, f"{what} {name}/{regime}")


def true_rho(dense, x):
    K, b, _, _, W = dense
    r = b - K @ x
    return float(np.sqrt(r @ (r / W)))


def tricg(A, device=0, **kw):
    return tk.setup(A, tk.K2(), tk.KrylovBackend(device=device, method="tricg", **kw))


def solve_on(kkt, th, rp, rd, xp, xd):
    tk.update(kkt, th, rp, rd)
    dx = np.zeros(kkt.n); dy = np.zeros(kkt.m)
    tk.solve(dx, dy, kkt, xp, xd)
    return dx, dy


@functools.lru_cache(maxsize=None)
def device_solution(name, regime):
    """one solve on the device per input row, shared by the tests that look at it: (dx, dy, stats)"""
    kkt = tricg(matrix(name))
    dx, dy = solve_on(kkt, *data(name, regime))
    st = kkt.stats()
    kkt.close()
    return dx, dy, st


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _raw_create(A, **fields):
    L = _lib.lib()
    A = sp.csc_matrix(A); A.sort_indices()
    m, n = A.shape
    opt = _lib.Options(); L.tlpk_default_options(ctypes.byref(opt))
    opt.device = -1
    opt.krylov = KRYLOV
    opt.system = _lib.SYSTEM_K2
    keep = []
    for k, v in fields.items():
        if isinstance(v, np.ndarray):
            keep.append(v); v = _lib.as_p64(v)
        setattr(opt, k, v)
    h = ctypes.c_void_p()
    colptr = A.indptr.astype(np.int64); rowval = A.indices.astype(np.int64); nz = np.ascontiguousarray(A.data, dtype=np.float64)
    rc = L.tlpk_create(ctypes.byref(h), m, n, _lib.as_p64(colptr), _lib.as_p64(rowval), _lib.as_pd(nz), 0, ctypes.byref(opt))
    return rc, h, L.tlpk_last_create_error().decode()


def test_analyse_only_create_takes_tricg_on_k2_only():
    assert KRYLOV == 32
    rc, h, _ = _raw_create(matrix("r30x50"))
    assert rc == _lib.OK and h
    _lib.lib().tlpk_destroy(h)
    rc, h, msg = _raw_create(matrix("r30x50"), system=_lib.SYSTEM_K1)
    assert rc == _lib.BADARG and not h and "krylov" in msg


def test_a_preconditioner_is_refused():
    rc, h, msg = _raw_create(matrix("r30x50"), krylov_precond=_lib.PRECOND_JACOBI)
    assert rc == _lib.BADARG and not h and "krylov_precond" in msg


@pytest.mark.parametrize("system", [_lib.SYSTEM_K1, _lib.SYSTEM_K2])
def test_trimr_is_reserved_and_refused(system):
    rc, h, msg = _raw_create(matrix("r30x50"), krylov=33, system=system)
    assert rc == _lib.BADARG and not h and msg


@pytest.mark.parametrize("fields", [
    dict(nranks=2), dict(dense_cols=1), dict(refine_steps=1), dict(user_perm=np.arange(30, dtype=np.int64)), dict(krylov_precond=2), dict(krylov_itmax=-1),
    dict(krylov_atol=-1.0), dict(krylov_rtol=float("nan")),
], ids=lambda f: ",".join(f"{k}" if isinstance(v, np.ndarray) else f"{k}={v}" for k, v in f.items()))
def test_create_refuses(fields):
    rc, h, msg = _raw_create(matrix("r30x50"), **fields)
    assert rc == _lib.BADARG and not h and msg


def test_struct_sizes_are_unchanged():
    assert ctypes.sizeof(_lib.Options) == 136 and ctypes.sizeof(_lib.Stats) == 304          # as before the method existed: no new field


def test_backend_object():
    assert tk.KrylovBackend(method="tricg").method == "tricg"
    with pytest.raises(ValueError):
        tk.KrylovBackend(method="trimr")
    with pytest.raises(ValueError):
        tk.KrylovBackend(method="tricg", precond="jacobi")
    A = matrix("r30x50")
    with pytest.raises(TypeError):
        tk.setup(A, tk.K1(), tk.KrylovBackend(device=-1, method="tricg"))
    from tulip_jl_amd.hsd_device import DeviceHSD
    from tulip_jl_amd.mpc_device import DeviceMPC
    m, n = A.shape
    args = (A, np.ones(m), np.ones(n), np.zeros(n), np.full(n, np.inf))
    for loop in (DeviceHSD, DeviceMPC):
        with pytest.raises(TypeError):
            loop(*args, system="K1", backend=tk.KrylovBackend(device=-1, method="tricg"))
        with pytest.raises(RuntimeError, match="no HIP device"):          # accepted: the analyse-only handle is made, loading the LP needs a device
            loop(*args, system="K2", backend=tk.KrylovBackend(device=-1, method="tricg"))


def test_backend_text():
    A = matrix("r30x50")
    assert tk.backend(tricg(A, device=-1)) == "HIP (gfx950) TriCG"
    assert tk.linear_system(tricg(A, device=-1)) == "Augmented system (K2)" == tk.linear_system(tk.setup(A, tk.K2(), tk.Backend(device=-1)))


@pytest.mark.parametrize("name", ["fixture", "r30x50", "r500"])
def test_analyse_only_handle_has_no_symbolic_structure(name):
    A = matrix(name)
    kkt = tricg(A, device=-1)
    st = kkt.stats()
    assert (st["m"], st["n"], st["nnzA"]) == (A.shape[0], A.shape[1], A.nnz)
    for key in ("nnzS", "nnzL", "nnzL_stored", "n_pairs", "n_supernodes", "flops_chol", "flops_panel", "flops_update", "flops_update_alg", "flops_syrk"):
        assert st[key] == 0, key
    assert (kkt.perm() == np.arange(A.shape[0] + A.shape[1])).all()          # the n + m nodes of K2, nothing reordered
    for what in ("s_colptr", "s_rowidx", "etree", "colcount", "rowidx", "pair_ptr", "factor_launches", "fwd_launches", "bwd_launches", "front_f"):
        arr = kkt.symbolic(what)
        assert arr.size == 0 or (what == "pair_ptr" and arr.tolist() == [0]), what
    for key in ("krylov_iters", "krylov_iters_total", "krylov_converged", "krylov_resid0", "krylov_resid"):
        assert st[key] == 0


def test_numeric_calls_need_a_device_and_there_is_no_factor():
    A = matrix("r30x50")
    kkt = tricg(A, device=-1)
    L = _lib.lib()
    th, rp, rd, xp, xd = data("r30x50", "unit")
    assert L.tlpk_update(kkt._h, _lib.as_pd(th), _lib.as_pd(rp), _lib.as_pd(rd)) == _lib.NO_DEVICE
    assert L.tlpk_solve(kkt._h, _lib.as_pd(np.zeros(50)), _lib.as_pd(np.zeros(30)), _lib.as_pd(xp), _lib.as_pd(xd)) == _lib.NO_DEVICE
    buf = np.zeros(8)
    assert L.tlpk_get_factor(kkt._h, _lib.as_pd(buf), 8) == _lib.BADARG and b"no factor" in L.tlpk_last_error(kkt._h)
    p = ctypes.c_void_p(); cnt = ctypes.c_int64()
    for name, args in [("tlpk_update_local", (None, None, None)), ("tlpk_solve_local", (None, None)), ("tlpk_solve2_local", (None,) * 4),
                       ("tlpk_refine_local", (None,) * 4), ("tlpk_root_panel", (ctypes.byref(p), ctypes.byref(cnt)))]:
        assert getattr(L, name)(kkt._h, *args) == _lib.BADARG, name
        assert b"matrix-free" in L.tlpk_last_error(kkt._h), name


def test_memory_gate_counts_a_and_the_tricg_vectors():
    A = matrix("r500")
    m, n = A.shape
    need = 36 * A.nnz + 136 * n + 168 * m + 65536          # include/tlpk.h / tlpk_api.cpp: krylov_bytes
    with pytest.raises(tk.OutOfMemoryError) as e:
        tricg(A, device=-1, mem_budget_bytes=need - 1)
    assert "bytes" in str(e.value)
    tricg(A, device=-1, mem_budget_bytes=need).close()
    rc, h, _ = _raw_create(A, mem_budget_bytes=need - 1)
    assert rc == _lib.TOO_LARGE
    rc, h, _ = _raw_create(A, mem_budget_bytes=need)
    assert rc == _lib.OK and h
    _lib.lib().tlpk_destroy(h)


@pytest.mark.parametrize("mat,reg", CONVERGING, ids=IDS)
def test_restatement_against_lapack(mat, reg):
    ref = assert_good_input(mat, reg)
    check_solution(mat, reg, ref["x"], ref["iters"], "restatement")
    g = gap_bound(mat, reg, ref["x"], ref["iters"])
    true = true_rho(dense_reference(mat, reg), ref["x"])
    print(f"  rho_k={ref['resid']:.3e} true rho={true:.3e} g={g:.3e}")
    assert abs(ref["resid"] - true) <= g


@pytest.mark.parametrize("zero", ["xi_p", "xi_d"])
def test_restatement_with_a_zero_first_lanczos_vector(zero):
    A = matrix("r30x50")
    th, rp, rd, xp, xd = data("r30x50", "unit")
    xp, xd = (np.zeros_like(xp), xd) if zero == "xi_p" else (xp, np.zeros_like(xd))
    ref = tricg_restatement(A, th, rp, rd, xp, xd)
    assert ref["converged"] and ref["iters"] <= ref["itmax"] // 2
    dense = _dense(A, th, rp, rd, xp, xd)
    _check(dense, ref["x"], ref["iters"], f"restatement r30x50/unit, {zero} = 0")
    assert abs(ref["resid"] - true_rho(dense, ref["x"])) <= _gap(dense, ref["x"], ref["iters"])


def test_restatement_counts_of_the_table():
    got = {(mat, reg): restated(mat, reg)["iters"] for mat, reg in CONVERGING}
    assert got == dict(zip(CONVERGING, COUNTS))
    assert restated("r30x50", "mid")["itmax"] == 160
    stalled = restated("r40x10", "mid")
    assert not stalled["converged"] and stalled["iters"] == 100 == stalled["itmax"]


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reference_conformance_fixture():
    A = matrix("fixture")
    kkt = tricg(A)
    rp_norm, rd_norm = tk.run_ls_tests(A, kkt)          # both residuals <= sqrt(eps)
    st = kkt.stats()
    print(f"fixture: residuals {rp_norm:.3e}, {rd_norm:.3e} in {st['krylov_iters']} iterations")
    assert rp_norm <= SQRT_EPS and rd_norm <= SQRT_EPS and st["krylov_converged"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("mat,reg", CONVERGING, ids=IDS)
def test_stopping_rule_is_honoured(mat, reg):
    assert_good_input(mat, reg)
    dx, dy, st = device_solution(mat, reg)
    x = np.concatenate([dx, dy])
    dense = dense_reference(mat, reg)
    _, b, _, _, W = dense
    g = gap_bound(mat, reg, x, st["krylov_iters"])
    rho = true_rho(dense, x); rho0 = float(np.sqrt(b @ (b / W)))
    tol = SQRT_EPS + SQRT_EPS * rho0
    print(f"{mat}/{reg}: k={st['krylov_iters']} true rho={rho:.3e} rho_k={st['krylov_resid']:.3e} tol={tol:.3e} g={g:.3e}")
    assert st["krylov_converged"] == 1 and st["krylov_resid"] <= tol
    assert rho <= tol + g
    assert abs(st["krylov_resid0"] - rho0) <= 1e-12 * rho0 + 1e-300


@pytest.mark.gpu
@pytest.mark.parametrize("mat,reg", CONVERGING, ids=IDS)
def test_solution(mat, reg):
    assert_good_input(mat, reg)
    dx, dy, st = device_solution(mat, reg)
    assert np.isfinite(dx).all() and np.isfinite(dy).all()
    check_solution(mat, reg, np.concatenate([dx, dy]), st["krylov_iters"], "device")


@pytest.mark.gpu
@pytest.mark.parametrize("mat,reg", CONVERGING, ids=IDS)
def test_iteration_count(mat, reg):
    ref = assert_good_input(mat, reg)
    _, _, st = device_solution(mat, reg)
    print(f"{mat}/{reg}: device {st['krylov_iters']} iterations, restatement {ref['iters']} (itmax {ref['itmax']})")
    assert 0 <= st["krylov_iters"] <= ref["itmax"]
    assert st["krylov_iters"] == st["krylov_iters_total"]


@pytest.mark.gpu
def test_not_converged_is_reported_not_hidden():
    ref = restated("r40x10", "mid")
    assert not ref["converged"] and ref["iters"] == 100            # the input guard of this test: the restatement stalls too
    A = matrix("r40x10")
    kkt = tricg(A)
    dx, dy = solve_on(kkt, *data("r40x10", "mid"))                  # returns: TLPK_OK
    st = kkt.stats()
    assert st["krylov_iters"] == 100 == 2 * sum(A.shape) and st["krylov_converged"] == 0
    assert kkt.symbolic("krylov_unsolved")[0] == 1
    assert np.isfinite(dx).all() and np.isfinite(dy).all()
    # the same handle, new update, data it can solve
    assert_good_input("r40x10", "unit")
    dx, dy = solve_on(kkt, *data("r40x10", "unit"))
    st = kkt.stats()
    assert st["krylov_converged"] == 1 and st["krylov_iters"] == st["krylov_iters_total"]
    check_solution("r40x10", "unit", np.concatenate([dx, dy]), st["krylov_iters"], "device, after a stalled solve")
    # itmax is honoured exactly
    assert restated("r500", "unit")["iters"] > 5
    k5 = tricg(matrix("r500"), itmax=5)
    solve_on(k5, *data("r500", "unit"))
    st = k5.stats()
    assert st["krylov_iters"] == 5 and st["krylov_converged"] == 0


@pytest.mark.gpu
def test_an_update_that_is_not_quasi_definite_is_refused():
    A = matrix("r30x50")
    m, n = A.shape
    th, rp, rd, xp, xd = data("r30x50", "unit")
    assert_good_input("r30x50", "unit")
    kkt = tricg(A)
    L = _lib.lib()

    def raw_update(th_, rp_, rd_):
        return L.tlpk_update(kkt._h, _lib.as_pd(np.ascontiguousarray(th_)), _lib.as_pd(np.ascontiguousarray(rp_)), _lib.as_pd(np.ascontiguousarray(rd_)))

    def raw_solve():
        return L.tlpk_solve(kkt._h, _lib.as_pd(np.zeros(n)), _lib.as_pd(np.zeros(m)), _lib.as_pd(xp), _lib.as_pd(xd))

    th0 = th.copy(); rp0 = rp.copy(); th0[17] = 0.0; rp0[17] = 0.0; th0[33] = 0.0; rp0[33] = 0.0          # the smallest one is reported
    assert raw_update(th0, rp0, rd) == _lib.NOT_POSDEF
    assert kkt.stats()["fail_col"] == 17 and b"not quasi-definite" in L.tlpk_last_error(kkt._h)
    assert raw_solve() == _lib.NOT_FACTORED
    rd0 = rd.copy(); rd0[4] = 0.0
    assert raw_update(th, rp, rd0) == _lib.NOT_POSDEF
    assert kkt.stats()["fail_col"] == n + 4
    assert raw_solve() == _lib.NOT_FACTORED
    rd0[4] = float("nan")
    with pytest.raises(tk.PosDefException):
        tk.update(kkt, th, rp, rd0)
    assert kkt.stats()["fail_col"] == n + 4
    # a valid update: the handle solves as if nothing had happened
    dx, dy = solve_on(kkt, th, rp, rd, xp, xd)
    st = kkt.stats()
    assert st["krylov_converged"] == 1 and st["fail_col"] == -1
    check_solution("r30x50", "unit", np.concatenate([dx, dy]), st["krylov_iters"], "device, after a refused update")


@pytest.mark.gpu
def test_bitwise_contracts():
    A = matrix("long600")
    m, n = A.shape
    th, rp, rd, xp, xd = data("long600", "unit")
    assert_good_input("long600", "unit")
    kkt = tricg(A)
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
    f1, f2 = tricg(A), tricg(A)
    fx3, fy3 = solve_on(f1, th2, rp, rd, xp, xd)
    fx4, fy4 = solve_on(f2, th, rp, rd, xp, xd)
    assert (dx3 == fx3).all() and (dy3 == fy3).all() and (dx4 == fx4).all() and (dy4 == fy4).all()
    assert (dx4 == dx0).all() and (dy4 == dy0).all()


@pytest.mark.gpu
def test_set_values_equals_a_fresh_handle():
    A = matrix("r500")
    th, rp, rd, xp, xd = data("r500", "unit")
    B = A.copy(); B.data = A.data * np.linspace(0.5, 1.5, A.nnz)
    guard = tricg_restatement(B, th, rp, rd, xp, xd)
    assert guard["converged"] and guard["iters"] <= guard["itmax"] // 2
    kkt = tricg(A)
    solve_on(kkt, th, rp, rd, xp, xd)
    tk.set_values(kkt, B)
    assert _lib.lib().tlpk_solve(kkt._h, _lib.as_pd(np.zeros(A.shape[1])), _lib.as_pd(np.zeros(A.shape[0])), _lib.as_pd(xp), _lib.as_pd(xd)) == _lib.NOT_FACTORED
    dx, dy = solve_on(kkt, th, rp, rd, xp, xd)
    fx, fy = solve_on(tricg(B), th, rp, rd, xp, xd)
    assert (dx == fx).all() and (dy == fy).all()
    assert kkt.stats()["krylov_converged"] == 1


@pytest.mark.gpu
def test_profile_mode_times_the_solve_as_spmv():
    A = matrix("r500")
    assert_good_input("r500", "unit")
    kkt = tricg(A, profile=True)
    solve_on(kkt, *data("r500", "unit"))
    kt, st = kkt.kernel_times(), kkt.stats()
    assert kt["spmv"]["launches"] >= 3 and kt["spmv"]["ms"] > 0.0
    for cls in ("assemble", "extend_add", "potrf", "trsm", "update", "solve_fwd", "solve_bwd", "update_reduce", "chain"):
        assert kt[cls]["launches"] == 0, cls
    assert st["krylov_converged"] == 1
    # documented: launches_update = 1 (W, 1 / W and the check); launches_solve = 2 (set-up) + 3 per enqueued iteration
    assert st["launches_update"] == 1
    assert (st["launches_solve"] - 2) % 3 == 0 and st["launches_solve"] >= 2 + 3 * st["krylov_iters"]


class _RestatementBackend:
    """tricg_restatement behind the three calls tests/ipm_harness.py asks of a KKT backend"""

    def __init__(self, A):
        self.A, self.unsolved, self.solves, self.max_iters = A, 0, 0, 0

    def update(self, th, rp, rd):
        self.args = (th.copy(), rp.copy(), rd.copy())

    def solve(self, dx, dy, xp, xd):
        out = tricg_restatement(self.A, *self.args, xp, xd)
        dx[:] = out["dx"]; dy[:] = out["dy"]
        self.unsolved += not out["converged"]; self.solves += 1
        self.max_iters = max(self.max_iters, out["iters"])


def _restatement_run(path, algorithm):
    from ipm_harness import read_free_mps as read_ref, solve_lp
    made = []
    ref, _ = solve_lp(read_ref(path), lambda A: made.append(_RestatementBackend(A)) or made[-1], algorithm=algorithm)
    return ref, made[0]


HSD_STATUS = {"lpex_opt": "Trm_Optimal", "lpex_freevars": "Trm_Optimal", "lpex_inf": "Trm_PrimalInfeasible", "lpex_ubd": "Trm_DualInfeasible"}
HSD_ALL_SOLVED = {"lpex_opt": True, "lpex_freevars": True, "lpex_inf": False, "lpex_ubd": True}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HSD_STATUS))
def test_device_resident_hsd(name):
    """lpex_inf: the rule measures the residual in the Rd^-1 norm and Rd falls to 1e-6; the restatement leaves 11 of its 20 solves at
    itmax = 10 and still ends in Trm_PrimalInfeasible.  There the status alone is asserted."""
    from tulip_jl_amd.hsd_device import DeviceHSD
    from tulip_jl_amd.problem import read_free_mps, standard_form
    path = os.path.join(GOLDEN, name + ".mps")
    ref, be = _restatement_run(path, "hsd")
    assert ref.status == HSD_STATUS[name] and (be.unsolved == 0) == HSD_ALL_SOLVED[name], "bad test input: the restatement does not behave as recorded"
    d = standard_form(read_free_mps(path))
    direct = DeviceHSD(d.A, d.b, d.c, d.l, d.u, c0=d.c0, objsense_min=d.objsense, system="K2", device=0).optimize()
    assert direct.status == HSD_STATUS[name]
    opt = DeviceHSD(d.A, d.b, d.c, d.l, d.u, c0=d.c0, objsense_min=d.objsense, system="K2", backend=tk.KrylovBackend(method="tricg")).optimize()
    print(f"{name}: {opt.status} in {opt.niter} iterations, z = {opt.primal_objective!r} (direct K2 {direct.primal_objective!r}), "
          f"{opt.timers['n_solve']} solves, {opt.kkt.symbolic('krylov_unsolved')[0]} unsolved; restatement: {ref.status}, {be.unsolved} of {be.solves} "
          f"unsolved, at most {be.max_iters} TriCG iterations per solve")
    assert opt.status == HSD_STATUS[name]
    if opt.status == "Trm_Optimal":
        assert abs(opt.primal_objective - direct.primal_objective) <= 1e-6 * (1 + abs(direct.primal_objective))
    if be.unsolved == 0:
        assert opt.kkt.symbolic("krylov_unsolved")[0] == 0          # every solve met the stopping rule
    assert opt.timers["n_solve"] > 0


@pytest.mark.gpu
def test_device_resident_mpc():
    from tulip_jl_amd.mpc_device import DeviceMPC
    from tulip_jl_amd.problem import read_free_mps, standard_form
    path = os.path.join(GOLDEN, "lpex_opt.mps")
    ref, be = _restatement_run(path, "mpc")
    assert ref.status == "Trm_Optimal" and be.unsolved == 0, "bad test input: the restatement does not solve it"
    d = standard_form(read_free_mps(path))
    direct = DeviceMPC(d.A, d.b, d.c, d.l, d.u, c0=d.c0, objsense_min=d.objsense, system="K2", device=0).optimize()
    opt = DeviceMPC(d.A, d.b, d.c, d.l, d.u, c0=d.c0, objsense_min=d.objsense, system="K2", backend=tk.KrylovBackend(method="tricg")).optimize()
    print(f"MPC lpex_opt: {opt.status} in {opt.niter} iterations, z = {opt.primal_objective!r} (direct K2 {direct.status}, {direct.primal_objective!r}), "
          f"{opt.kkt.symbolic('krylov_unsolved')[0]} unsolved")
    assert opt.status == direct.status == "Trm_Optimal"
    assert abs(opt.primal_objective - direct.primal_objective) <= 1e-6 * (1 + abs(direct.primal_objective))
    assert opt.kkt.symbolic("krylov_unsolved")[0] == 0
