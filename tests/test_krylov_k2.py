"""Matrix-free K2 backend (tlpk_options.krylov = TLPK_KRYLOV_MINRES): preconditioned MINRES on [-E A'; A Rd] [dx; dy] = [xi_d; xi_p] on the device.

The comparator is `minres_restatement` below: the algorithm of include/tlpk.h / DESIGN.md section 1b''''' in numpy (Paige & Saunders: a Lanczos
recurrence and one Givens rotation per step; solved when phibar <= atol + rtol beta1; tired after itmax = 2 (m + n) iterations; r'M^-1 r < 0 ends
it unsolved).  Every test that relies on convergence first asserts that the RESTATEMENT converges within half of itmax on its input.  Inputs: matrices
of the table of tests/test_krylov.py; the regime "unreg" is "unit" with every 7th theta^-1 + Rp set to 0 and Rd = 0, which the K1 handle cannot take.

Restatement iteration counts, none / Jacobi: fixture 2 / 2, r1x5 3 / 3, r40x10 20 / 22, r30x50 39 / 37, r500 72 / 47, long600 98 / 53,
ba1220 88 / 47, r500 mid - / 623 of 3400 (none: stops at itmax = 3400), r500 unreg 891 / 605."""
import ctypes
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import tulip_jl_amd as tk
from tulip_jl_amd import _lib
from helpers import DevBuf, block_angular, ipm_like_data, random_lp_matrix

EPS = float(np.finfo(np.float64).eps)
SQRT_EPS = float(np.sqrt(EPS))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs (the constructions of tests/test_krylov.py's table)
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
# (matrix, regime, preconditioner) of every row that converges
CONVERGING = [(mat, "unit", pre) for mat in ("fixture", "r1x5", "r40x10", "r30x50", "r500", "long600", "ba1220") for pre in (None, "jacobi")]
CONVERGING += [("r500", "mid", "jacobi"), ("r500", "unreg", None), ("r500", "unreg", "jacobi")]
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
    if regime == "unreg":
        th, rp, rd, xp, xd = (a.copy() for a in ipm_like_data(m, n, 1, "unit"))
        th[::7] = 0.0; rp[::7] = 0.0; rd[:] = 0.0          # free variables without primal regularisation, no dual regularisation
        return th, rp, rd, xp, xd
    return ipm_like_data(m, n, 1, regime)


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def block_diagonal(A, E, rd):
    """M = diag(E_j, s_i), s_i = sum_{j: E_j > 0} A_ij^2 / E_j + Rd_i; an entry that is 0 is replaced by 1"""
    A = sp.csr_matrix(A)
    Einv = np.where(E > 0.0, 1.0 / np.where(E > 0.0, E, 1.0), 0.0)
    M = np.concatenate([E, A.multiply(A) @ Einv + rd])
    M[M == 0.0] = 1.0
    return M


def minres_restatement(A, th, rp, rd, xp, xd, precond=None, itmax=0, atol=0.0, rtol=0.0):
    """-> dict(dx, dy, x, iters, converged, resid0, resid, itmax)"""
    A = sp.csr_matrix(A)
    m, n = A.shape
    N = n + m
    At = A.T.tocsr()
    E = th + rp
    itmax = itmax or 2 * N
    atol = atol or SQRT_EPS; rtol = rtol or SQRT_EPS
    Minv = 1.0 / block_diagonal(A, E, rd) if precond == "jacobi" else np.ones(N)

    def K(v):
        return np.concatenate([-E * v[:n] + At @ v[n:], A @ v[:n] + rd * v[n:]])

    r1 = np.concatenate([xd, xp]); y = Minv * r1
    beta1 = float(np.sqrt(r1 @ y)); phibar = beta1; tol = atol + rtol * beta1
    solved = beta1 <= tol
    oldb = 0.0; beta = beta1; dbar = 0.0; eps = 0.0; cs = -1.0; sn = 0.0
    x = np.zeros(N); w = np.zeros(N); w2 = np.zeros(N); r2 = r1
    k = 0
    while not solved and k < itmax:
        k += 1
        v = y / beta
        y = K(v)
        if k >= 2:
            y = y - (beta / oldb) * r1
        alpha = float(v @ y)
        y = y - (alpha / beta) * r2
        r1 = r2; r2 = y; y = Minv * r2
        oldb = beta
        g = float(r2 @ y)
        if not (g >= 0.0) or not np.isfinite(g):
            break
        beta = float(np.sqrt(g))
        oldeps = eps; delta = cs * dbar + sn * alpha; gbar = sn * dbar - cs * alpha; eps = sn * beta; dbar = -cs * beta
        gamma = max(float(np.hypot(gbar, beta)), EPS); cs = gbar / gamma; sn = beta / gamma; phi = cs * phibar; phibar = sn * phibar
        w1 = w2; w2 = w; w = (v - oldeps * w1 - delta * w2) / gamma
        x = x + phi * w
        solved = phibar <= tol
        if beta == 0.0:
            break
    return dict(dx=x[:n].copy(), dy=x[n:].copy(), x=x, iters=k, converged=bool(solved), resid0=beta1, resid=float(phibar), itmax=itmax)


@functools.lru_cache(maxsize=None)
def restated(name, regime, precond):
    return minres_restatement(matrix(name), *data(name, regime), precond=precond)


@functools.lru_cache(maxsize=None)
def dense_reference(name, regime):
    """K (sparse), b, x* = K \\ b (LAPACK), sigma_min(K), the block diagonal M"""
    A = matrix(name)
    th, rp, rd, xp, xd = data(name, regime)
    E = th + rp
    K = sp.bmat([[-sp.diags(E), A.T], [A, sp.diags(rd)]]).tocsr()
    Kd = K.toarray()
    b = np.concatenate([xd, xp])
    return K, b, np.linalg.solve(Kd, b), float(np.abs(np.linalg.eigvalsh(Kd)).min()), block_diagonal(A, E, rd)


def assert_good_input(name, regime, precond):
    ref = restated(name, regime, precond)
    assert ref["converged"] and ref["iters"] <= ref["itmax"] // 2, f"bad test input {name}/{regime}/{precond}: the restatement needs {ref['iters']} of {ref['itmax']}"
    return ref


def gap_bound(name, regime, precond, x, k):
    """g = 4 k eps (|K|inf |x|inf + |b|inf) sqrt(N max_i M^-1_i): tests/test_krylov.py's gap_bound with K, x, N in place of S, dy, m"""
    K, b, _, _, M = dense_reference(name, regime)
    N = K.shape[0]
    Minv = 1.0 / M if precond == "jacobi" else np.ones(N)
    k_inf = float(abs(K).sum(axis=1).max())
    return 4.0 * k * EPS * (k_inf * np.abs(x).max(initial=0.0) + np.abs(b).max(initial=0.0)) * np.sqrt(N * Minv.max()), Minv


def check_solution(name, regime, precond, x, k, what):
    """|x - x*|2 <= (tol + g) sqrt(max M) / sigma_min(K)"""
    _, b, x_star, sig_min, _ = dense_reference(name, regime)
    g, Minv = gap_bound(name, regime, precond, x, k)
    beta1 = float(np.sqrt(b @ (Minv * b)))
    bound = ((SQRT_EPS + SQRT_EPS * beta1) + g) * np.sqrt((1.0 / Minv).max()) / sig_min
    err = float(np.linalg.norm(x - x_star))
    print(f"{what} {name}/{regime}/{precond}: k={k} |x - x*|2={err:.3e} bound={bound:.3e} (g={g:.3e}, sigma_min={sig_min:.3e})")
    assert err <= bound


def minres(A, device=0, **kw):
    return tk.setup(A, tk.K2(), tk.KrylovBackend(device=device, method="minres", **kw))


def solve_on(kkt, th, rp, rd, xp, xd):
    tk.update(kkt, th, rp, rd)
    dx = np.zeros(kkt.n); dy = np.zeros(kkt.m)
    tk.solve(dx, dy, kkt, xp, xd)
    return dx, dy


@functools.lru_cache(maxsize=None)
def device_solution(name, regime, precond):
    """one solve on the device per input row, shared by the tests that look at it: (dx, dy, stats)"""
    kkt = minres(matrix(name), precond=precond)
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
    opt.krylov = 16
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


def test_analyse_only_create_takes_minres_on_k2_only():
    assert _lib.KRYLOV_MINRES == 16
    rc, h, _ = _raw_create(matrix("r30x50"))
    assert rc == _lib.OK and h
    _lib.lib().tlpk_destroy(h)
    rc, h, msg = _raw_create(matrix("r30x50"), system=_lib.SYSTEM_K1)
    assert rc == _lib.BADARG and not h and "krylov" in msg
    rc, h, msg = _raw_create(matrix("r30x50"), krylov=_lib.KRYLOV_CG)          # CG on K2: refused as before
    assert rc == _lib.BADARG and not h and "krylov" in msg and "not implemented" not in msg


@pytest.mark.parametrize("value", [2, 3, 15, 17])
@pytest.mark.parametrize("system", [_lib.SYSTEM_K1, _lib.SYSTEM_K2])
def test_unknown_methods_are_refused(value, system):
    rc, h, msg = _raw_create(matrix("r30x50"), krylov=value, system=system)
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
    assert tk.KrylovBackend().method == "cg" and tk.KrylovBackend(method="minres").method == "minres"
    with pytest.raises(ValueError):
        tk.KrylovBackend(method="gmres")
    A = matrix("r30x50")
    with pytest.raises(TypeError):
        tk.setup(A, tk.K1(), tk.KrylovBackend(device=-1, method="minres"))
    with pytest.raises(TypeError):
        tk.setup(A, tk.K2(), tk.KrylovBackend(device=-1))
    from tulip_jl_amd.hsd_device import DeviceHSD
    m, n = A.shape
    args = (A, np.ones(m), np.ones(n), np.zeros(n), np.full(n, np.inf))
    with pytest.raises(TypeError):
        DeviceHSD(*args, system="K1", backend=tk.KrylovBackend(device=-1, method="minres"))
    with pytest.raises(TypeError):
        DeviceHSD(*args, system="K2", backend=tk.KrylovBackend(device=-1))


def test_backend_text():
    A = matrix("r30x50")
    assert tk.backend(minres(A, device=-1)) == "HIP (gfx950) MINRES"
    assert tk.backend(minres(A, device=-1, precond="jacobi")) == "HIP (gfx950) MINRES, Jacobi"
    assert tk.linear_system(minres(A, device=-1)) == "Augmented system (K2)" == tk.linear_system(tk.setup(A, tk.K2(), tk.Backend(device=-1)))


@pytest.mark.parametrize("name", ["fixture", "r30x50", "r500"])
def test_analyse_only_handle_has_no_symbolic_structure(name):
    A = matrix(name)
    kkt = minres(A, device=-1)
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
    kkt = minres(A, device=-1)
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


def test_memory_gate_counts_a_and_the_minres_vectors():
    A = matrix("r500")
    m, n = A.shape
    need = 36 * A.nnz + 144 * n + 176 * m + 65536          # include/tlpk.h / tlpk_api.cpp: krylov_bytes
    with pytest.raises(tk.OutOfMemoryError) as e:
        minres(A, device=-1, mem_budget_bytes=need - 1)
    assert "bytes" in str(e.value)
    minres(A, device=-1, mem_budget_bytes=need).close()
    rc, h, _ = _raw_create(A, mem_budget_bytes=need - 1)
    assert rc == _lib.TOO_LARGE


@pytest.mark.parametrize("mat,reg,pre", CONVERGING, ids=IDS)
def test_restatement_against_lapack(mat, reg, pre):
    ref = assert_good_input(mat, reg, pre)
    check_solution(mat, reg, pre, ref["x"], ref["iters"], "restatement")
    if pre is None:
        K, b, _, _, _ = dense_reference(mat, reg)
        g, _ = gap_bound(mat, reg, pre, ref["x"], ref["iters"])
        true = float(np.linalg.norm(b - K @ ref["x"]))
        print(f"  phibar={ref['resid']:.3e} true |b - K x|2={true:.3e} g={g:.3e}")
        assert abs(ref["resid"] - true) <= g


def test_restatement_counts_of_the_table():
    got = {(mat, reg, pre): restated(mat, reg, pre)["iters"] for mat, reg, pre in CONVERGING}
    want = dict(zip(CONVERGING, [2, 2, 3, 3, 20, 22, 39, 37, 72, 47, 98, 53, 88, 47, 623, 891, 605]))
    assert got == want
    stalled = restated("r500", "mid", None)
    assert not stalled["converged"] and stalled["iters"] == 3400


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reference_conformance_fixture():
    A = matrix("fixture")
    for pre in (None, "jacobi"):
        kkt = minres(A, precond=pre)
        rp_norm, rd_norm = tk.run_ls_tests(A, kkt)          # both residuals <= sqrt(eps)
        st = kkt.stats()
        print(f"fixture/{pre}: residuals {rp_norm:.3e}, {rd_norm:.3e} in {st['krylov_iters']} iterations")
        assert rp_norm <= SQRT_EPS and rd_norm <= SQRT_EPS and st["krylov_converged"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("mat,reg,pre", CONVERGING, ids=IDS)
def test_stopping_rule_is_honoured(mat, reg, pre):
    assert_good_input(mat, reg, pre)
    dx, dy, st = device_solution(mat, reg, pre)
    x = np.concatenate([dx, dy])
    K, b, _, _, _ = dense_reference(mat, reg)
    g, Minv = gap_bound(mat, reg, pre, x, st["krylov_iters"])
    r = b - K @ x
    rho = float(np.sqrt(r @ (Minv * r))); beta1 = float(np.sqrt(b @ (Minv * b)))
    tol = SQRT_EPS + SQRT_EPS * beta1
    print(f"{mat}/{reg}/{pre}: k={st['krylov_iters']} true rho={rho:.3e} phibar={st['krylov_resid']:.3e} tol={tol:.3e} g={g:.3e}")
    assert st["krylov_converged"] == 1 and st["krylov_resid"] <= tol
    assert rho <= tol + g
    assert abs(st["krylov_resid0"] - beta1) <= 1e-12 * beta1 + 1e-300


@pytest.mark.gpu
@pytest.mark.parametrize("mat,reg,pre", CONVERGING, ids=IDS)
def test_solution(mat, reg, pre):
    assert_good_input(mat, reg, pre)
    dx, dy, st = device_solution(mat, reg, pre)
    assert np.isfinite(dx).all() and np.isfinite(dy).all()
    check_solution(mat, reg, pre, np.concatenate([dx, dy]), st["krylov_iters"], "device")


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
    assert not ref["converged"] and ref["iters"] == 3400            # the input guard of this test: the restatement stalls too
    A = matrix("r500")
    kkt = minres(A)
    dx, dy = solve_on(kkt, *data("r500", "mid"))                    # returns: TLPK_OK
    st = kkt.stats()
    assert st["krylov_iters"] == 3400 == 2 * sum(A.shape) and st["krylov_converged"] == 0
    assert kkt.symbolic("krylov_unsolved")[0] == 1
    assert np.isfinite(dx).all() and np.isfinite(dy).all()
    # the same handle, new update, data it can solve
    assert_good_input("r500", "unit", None)
    dx, dy = solve_on(kkt, *data("r500", "unit"))
    st = kkt.stats()
    assert st["krylov_converged"] == 1 and st["krylov_iters"] == st["krylov_iters_total"]
    check_solution("r500", "unit", None, np.concatenate([dx, dy]), st["krylov_iters"], "device, after a stalled solve")
    # itmax is honoured exactly
    k5 = minres(A, itmax=5)
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
    kkt = minres(A, precond=pre)
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
    f1, f2 = minres(A, precond=pre), minres(A, precond=pre)
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
    guard = minres_restatement(B, th, rp, rd, xp, xd, precond=pre)
    assert guard["converged"] and guard["iters"] <= guard["itmax"] // 2
    kkt = minres(A, precond=pre)
    solve_on(kkt, th, rp, rd, xp, xd)
    tk.set_values(kkt, B)
    assert _lib.lib().tlpk_solve(kkt._h, _lib.as_pd(np.zeros(A.shape[1])), _lib.as_pd(np.zeros(A.shape[0])), _lib.as_pd(xp), _lib.as_pd(xd)) == _lib.NOT_FACTORED
    dx, dy = solve_on(kkt, th, rp, rd, xp, xd)
    fx, fy = solve_on(minres(B, precond=pre), th, rp, rd, xp, xd)
    assert (dx == fx).all() and (dy == fy).all()
    assert kkt.stats()["krylov_converged"] == 1


@pytest.mark.gpu
def test_profile_mode_times_the_solve_as_spmv():
    A = matrix("r500")
    assert_good_input("r500", "unit", "jacobi")
    kkt = minres(A, precond="jacobi", profile=True)
    solve_on(kkt, *data("r500", "unit"))
    kt, st = kkt.kernel_times(), kkt.stats()
    assert kt["spmv"]["launches"] >= 3 and kt["spmv"]["ms"] > 0.0
    for cls in ("assemble", "extend_add", "potrf", "trsm", "update", "solve_fwd", "solve_bwd", "update_reduce", "chain"):
        assert kt[cls]["launches"] == 0, cls
    assert st["krylov_converged"] == 1
    # documented: launches_update = 1 (E) + 1 (block diagonal); launches_solve = 2 (set-up) + 3 per enqueued iteration
    assert st["launches_update"] == 2 and st["launches_solve"] >= 2 + 2 * st["krylov_iters"]
    assert (st["launches_solve"] - 2) % 3 == 0 and st["launches_solve"] >= 2 + 3 * st["krylov_iters"]


class _RestatementBackend:
    """minres_restatement behind the three calls tests/ipm_harness.py asks of a KKT backend"""

    def __init__(self, A, precond):
        self.A, self.precond, self.unsolved, self.max_iters = A, precond, 0, 0

    def update(self, th, rp, rd):
        self.args = (th.copy(), rp.copy(), rd.copy())

    def solve(self, dx, dy, xp, xd):
        out = minres_restatement(self.A, *self.args, xp, xd, precond=self.precond)
        dx[:] = out["dx"]; dy[:] = out["dy"]
        self.unsolved += not out["converged"]
        self.max_iters = max(self.max_iters, out["iters"])


def _restatement_run(path, precond, algorithm):
    from ipm_harness import read_free_mps as read_ref, solve_lp
    made = []
    ref, _ = solve_lp(read_ref(path), lambda A: made.append(_RestatementBackend(A, precond)) or made[-1], algorithm=algorithm)
    return ref, made[0]


HSD_STATUS = {"lpex_opt": "Trm_Optimal", "lpex_freevars": "Trm_Optimal", "lpex_inf": "Trm_PrimalInfeasible", "lpex_ubd": "Trm_DualInfeasible"}


@pytest.mark.gpu
@pytest.mark.parametrize("pre", [None, "jacobi"])
@pytest.mark.parametrize("name", sorted(HSD_STATUS))
def test_device_resident_hsd(name, pre):
    """lpex_inf without a preconditioner is a marginal input: N = 5, itmax = 10, and the h-system of its last interior-point iteration needs 8 or 9
    iterations in the restatement.  A build that formed v = z / beta with a reciprocal multiplication left one of its 16 solves at itmax (phibar
    7.3e-08 against a tolerance of 4.5e-08); with the division of the restatement every solve meets the rule."""
    from tulip_jl_amd.hsd_device import DeviceHSD
    from tulip_jl_amd.problem import read_free_mps, standard_form
    path = os.path.join(GOLDEN, name + ".mps")
    ref, be = _restatement_run(path, pre, "hsd")
    assert ref.status == HSD_STATUS[name] and be.unsolved == 0, "bad test input: the restatement does not solve it"
    d = standard_form(read_free_mps(path))
    direct = DeviceHSD(d.A, d.b, d.c, d.l, d.u, c0=d.c0, objsense_min=d.objsense, system="K2", device=0).optimize()
    assert direct.status == HSD_STATUS[name]
    opt = DeviceHSD(d.A, d.b, d.c, d.l, d.u, c0=d.c0, objsense_min=d.objsense, system="K2",
                    backend=tk.KrylovBackend(method="minres", precond=pre)).optimize()
    print(f"{name}/{pre}: {opt.status} in {opt.niter} iterations, z = {opt.primal_objective!r} (direct K2 {direct.primal_objective!r}), "
          f"{opt.timers['n_solve']} solves; restatement: at most {be.max_iters} MINRES iterations per solve")
    assert opt.status == HSD_STATUS[name]
    if opt.status == "Trm_Optimal":
        assert abs(opt.primal_objective - direct.primal_objective) <= 1e-6 * (1 + abs(direct.primal_objective))
    assert opt.kkt.symbolic("krylov_unsolved")[0] == 0              # every solve met the stopping rule
    assert opt.timers["n_solve"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("pre", [None, "jacobi"])
def test_device_resident_mpc(pre):
    """lpex_opt with Jacobi is the case Jacobi-CG on K1 loses (DESIGN.md section 1b'''', limits)"""
    from tulip_jl_amd.mpc_device import DeviceMPC
    from tulip_jl_amd.problem import read_free_mps, standard_form
    path = os.path.join(GOLDEN, "lpex_opt.mps")
    ref, be = _restatement_run(path, pre, "mpc")
    assert ref.status == "Trm_Optimal" and be.unsolved == 0, "bad test input: the restatement does not solve it"
    d = standard_form(read_free_mps(path))
    direct = DeviceMPC(d.A, d.b, d.c, d.l, d.u, c0=d.c0, objsense_min=d.objsense, system="K2", device=0).optimize()
    opt = DeviceMPC(d.A, d.b, d.c, d.l, d.u, c0=d.c0, objsense_min=d.objsense, system="K2",
                    backend=tk.KrylovBackend(method="minres", precond=pre)).optimize()
    print(f"MPC lpex_opt/{pre}: {opt.status} in {opt.niter} iterations, z = {opt.primal_objective!r} (direct K2 {direct.status}, {direct.primal_objective!r})")
    assert opt.status == direct.status == "Trm_Optimal"
    assert abs(opt.primal_objective - direct.primal_objective) <= 1e-6 * (1 + abs(direct.primal_objective))
