"""Dense-matrix K1 backend (tlpk_create_dense / tk.DenseBackend): the counterpart of the reference's dense solver
(src/KKT/Dense/lapack.jl).  A is a dense column-major array; A*D*A' + Rd is formed by an fp64-MFMA SYRK straight into the one
front of the handle, factorised by the blocked dense Cholesky of the sparse handles and solved around two dense GEMVs.

CPU part: the analyse path that builds ONE front without a pattern of S or assembly lists (statistics, argument checks, a cap on
the host memory, and the exported factorisation schedule executed in numpy).  GPU part (-m gpu): factor and solutions against
numpy / LAPACK on the host, the contracts every handle keeps, and a matrix game solved end to end by the device-resident loops."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla

import tulip_jl_amd as tk
from emulate import Emulator, panels_to_dense_L, pk_off
from helpers import SQRT_EPS, DevBuf, ipm_like_data, kkt_residuals
from tulip_jl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LTOL, XTOL = 1e-11, 1e-9            # the project's tolerances (tests/test_gpu_parity.py: compare_with_oracle)


def dense_A(m, n, seed=0):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((m, n)))


def numpy_reference(A, th, rp, rd, xp, xd):
    """K = (A*D) @ A' + diag(rd), its Cholesky factor, and the Newton step through two triangular solves."""
    D = 1.0 / (th + rp)
    K = (A * D) @ A.T + np.diag(rd)
    L = np.linalg.cholesky(K)
    dy = sla.solve_triangular(L, xp + A @ (D * xd), lower=True)
    dy = sla.solve_triangular(L.T, dy, lower=False)
    dx = D * (A.T @ dy - xd)
    return K, L, dx, dy


def create_raw(m, n, A, lda, **fields):
    """tlpk_create_dense through ctypes: (return code, handle, message of a failed create)."""
    L = _lib.lib()
    opt = _lib.Options(); L.tlpk_default_options(ctypes.byref(opt)); opt.device = -1
    keep = []
    for k, v in fields.items():
        if isinstance(v, np.ndarray):
            keep.append(v); v = _lib.as_p64(v)
        setattr(opt, k, v)
    h = ctypes.c_void_p()
    rc = L.tlpk_create_dense(ctypes.byref(h), m, n, None if A is None else _lib.as_pd(A), lda, ctypes.byref(opt))
    return rc, h, L.tlpk_last_create_error().decode()


# ------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------
SHAPES_CPU = [(1, 5), (2, 4), (100, 37), (333, 1001), (800, 1600)]


@pytest.mark.parametrize("m,n", SHAPES_CPU)
def test_analyse_only_handle(m, n):
    A = dense_A(m, n)
    kkt = tk.setup(A, tk.K1(), tk.DenseBackend(device=-1))
    assert isinstance(kkt, tk.HIPNormalEquations)
    st = kkt.stats()
    assert (st["m"], st["n"], st["nnzA"]) == (m, n, m * n)
    assert st["nnzS"] == st["nnzL"] == m * (m + 1) // 2
    assert st["n_pairs"] == 0 and st["n_supernodes"] == 1 and st["max_front"] == m and st["n_dense_cols"] == 0
    assert st["flops_chol"] == float(sum(l * l for l in range(1, m + 1)))
    assert st["flops_syrk"] == float(n * m * (m + 1))
    assert (kkt.perm() == np.arange(m)).all()
    assert (kkt.symbolic("front_f") == [m]).all() and (kkt.symbolic("front_ns") == [m]).all()
    # no pattern of S, no assembly lists
    assert (kkt.symbolic("s_colptr") == np.zeros(m + 1)).all()
    for name in ("s_target", "s_diag_row", "pair_j", "s_rowidx"):
        assert len(kkt.symbolic(name)) == 0, name
    assert len(_lib.symbolic_array_f64(kkt._h, "pair_w")) == 0
    # the launch geometry of the dense kernels (tests/test_dense_shapes.py holds its rule): K parts x columns cover n, so do the chunks; the two leading dimensions
    split, kc, chunks, cw, dlda, plda = kkt.symbolic("dense_geometry").tolist()
    assert kc % 16 == 0 and (split - 1) * kc < n <= split * kc and (chunks - 1) * cw < n <= chunks * cw
    assert dlda == (m + 15) // 16 * 16 and plda == kkt.symbolic("front_lda")[0]
    th, rp, rd, xp, xd = ipm_like_data(m, n, 0)
    assert _lib.lib().tlpk_update(kkt._h, _lib.as_pd(th), _lib.as_pd(rp), _lib.as_pd(rd)) == _lib.NO_DEVICE
    # a sparse handle of the same (tiny) matrix reports flops_syrk = 0
    if m <= 2:
        assert tk.setup(A, tk.K1(), tk.Backend(device=-1)).stats()["flops_syrk"] == 0.0


def test_bad_arguments_return_no_handle_and_a_message():
    m, n = 6, 9
    A = dense_A(m, n)
    ones = np.zeros(m, dtype=np.int64)
    cases = {
        "A == NULL": dict(A=None),
        "lda < m": dict(lda=m - 1),
        "K2": dict(system=_lib.SYSTEM_K2),
        "nranks": dict(nranks=2),
        "row_block": dict(row_block=ones),
        "detect_blocks": dict(detect_blocks=1),
        "user_perm": dict(user_perm=np.arange(m, dtype=np.int64)),
        "dense_cols": dict(dense_cols=1),
        "refine_steps": dict(refine_steps=1),
    }
    for name, kw in cases.items():
        a = kw.pop("A", A); lda = kw.pop("lda", m)
        rc, h, msg = create_raw(m, n, a, lda, **kw)
        assert rc == _lib.BADARG and not h and msg, (name, rc, msg)
    rc, h, msg = create_raw(m, n, A, m)
    assert rc == _lib.OK and h and msg == ""
    # the split-phase calls and the multi-device create do not apply to such a handle
    L = _lib.lib()
    p = ctypes.c_void_p(); cnt = ctypes.c_int64()
    assert L.tlpk_update_local(h, 8, 8, 8) == _lib.BADARG and b"split-phase" in L.tlpk_last_error(h)
    assert L.tlpk_update_finish(h) == _lib.BADARG
    assert L.tlpk_solve_local(h, 8, 8) == _lib.BADARG
    assert L.tlpk_solve_finish(h, 8, 8, 8) == _lib.BADARG
    assert L.tlpk_root_panel(h, ctypes.byref(p), ctypes.byref(cnt)) == _lib.BADARG
    assert L.tlpk_root_rhs(h, ctypes.byref(p), ctypes.byref(cnt)) == _lib.BADARG
    L.tlpk_destroy(h)
    # Python front end: sparse matrices and K2 are type errors
    import scipy.sparse as sp
    with pytest.raises(TypeError):
        tk.setup(sp.csc_matrix(A), tk.K1(), tk.DenseBackend(device=-1))
    with pytest.raises(TypeError):
        tk.setup(A, tk.K2(), tk.DenseBackend(device=-1))


def test_memory_budget_is_checked_and_states_the_bytes():
    m, n = 512, 1024
    rc, h, msg = create_raw(m, n, dense_A(m, n), m, mem_budget_bytes=1 << 20)
    assert rc == _lib.TOO_LARGE and not h and "bytes" in msg
    rc, h, msg = create_raw(m, n, dense_A(m, n), m, mem_budget_bytes=1 << 20, keep_on_too_large=1)
    assert rc == _lib.TOO_LARGE and h                      # the live analyse-only handle that describes what did not fit
    st = _lib.Stats(); _lib.lib().tlpk_info(h, ctypes.byref(st))
    assert st.m == m and st.nnzL == m * (m + 1) // 2
    _lib.lib().tlpk_destroy(h)


def test_leading_dimension_does_not_change_the_analysis():
    m, n = 333, 1001
    A = dense_A(m, n)
    big = np.zeros((m + 11, n), order="F"); big[:m] = A
    k0 = tk.setup(A, tk.K1(), tk.DenseBackend(device=-1))
    k1 = tk.setup(big[:m], tk.K1(), tk.DenseBackend(device=-1))
    assert k1.A.base is big or k1.A is big[:m] or np.shares_memory(k1.A, big)          # passed as it is, not copied
    for name in ("perm", "front_f", "front_ns", "front_lda", "front_loff", "factor_launches", "fwd_launches", "bwd_launches", "potrf_tasks",
                 "trsm_tasks", "update_tasks", "reduce_tasks", "chain_items", "fwd_sweep_tasks", "bwd_sweep_tasks", "dense_geometry"):
        assert (k0.symbolic(name) == k1.symbolic(name)).all(), name
    # a C-ordered array is copied once into column-major storage
    k2 = tk.setup(np.ascontiguousarray(A), tk.K1(), tk.DenseBackend(device=-1))
    assert k2.A.flags.f_contiguous and (k2.A == A).all()


_MEM_CHILD = r"""
import resource, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import tulip_jl_amd as tk
m, n = 3000, 6000
A = np.empty((m, n), order="F")                 # filled in place, in slabs: the peak so far is A itself, not a temporary of its size
rng = np.random.default_rng(0)
for j in range(0, n, 250):
    A[:, j: j + 250] = rng.standard_normal((m, 250))
tk._lib.lib()
before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
kkt = tk.setup(A, tk.K1(), tk.DenseBackend(device=-1))
after = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
st = kkt.stats()
print("RSS", before, after, A.nbytes, st["nnzL"], st["n_pairs"])
"""


def test_host_memory_of_create_is_bounded_by_the_matrix():
    """A cap, not a measurement: creating the handle of a 3000 x 6000 matrix (144 MB) raises the peak RSS of the process by less
    than 4 x the bytes of A.  The sparse path would need 2.7e10 assembly-list entries for this shape (hundreds of GB)."""
    out = subprocess.run([sys.executable, "-c", _MEM_CHILD, ROOT], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    tag, before, after, nbytes, nnzL, n_pairs = [ln for ln in out.stdout.splitlines() if ln.startswith("RSS")][0].split()
    grown = (int(after) - int(before)) * 1024                # ru_maxrss is in KiB
    print(f"peak RSS grew by {grown / 1e6:.1f} MB for a matrix of {int(nbytes) / 1e6:.1f} MB")
    assert int(nnzL) == 3000 * 3001 // 2 and int(n_pairs) == 0
    assert grown < 4 * int(nbytes)


class DenseEmulator(Emulator):
    """tests/emulate.py's executor of the exported schedules, with numpy's tril(A*D*A' + Rd) put into the packed panel where the
    sparse handles run their list-driven assembly (the device runs k_dense_syrk there)."""

    def update(self, theta, regP, regD, stop_at_marker=False):
        A = np.asarray(self.kkt.A)
        self.D = 1.0 / (theta + regP)
        self.regD = np.asarray(regD, dtype=float)
        self.Lval[:] = np.nan                                # nothing may rely on a zero-fill
        self._P = {}
        assert len(self.f) == 1 and self.f[0] == self.ns[0] == self.m
        K = self.form_panel(A)
        self._svals = {}; self._upper_pending = {}; self.U = {}; self.fail_col = None
        self.chain_cnt[:] = 0
        for s_ in np.nonzero(self.single & (self.local != 0))[0]:      # k_single_factor (m = 1)
            self.Lval[self.loff[s_]] = np.sqrt(self.Lval[self.loff[s_]])
        self._resume = self._run(self.factor_launches, True)
        self.update_finish()
        return K

    def form_panel(self, A):
        """What stands for k_dense_syrk (tests/test_dense_shapes.py puts the device's tiles, K parts and slabs here): every stored entry is written."""
        K = (A * self.D) @ A.T + np.diag(self.regD)
        lda, loff = int(self.lda[0]), int(self.loff[0])
        for c in range(self.m):
            top = (c >> 6) << 6                              # first stored row of the column's 64-column slice
            a = loff + pk_off(lda, c)
            self.Lval[a + top: a + c] = 0.0
            self.Lval[a + c: a + self.m] = K[c:, c]
            self.Lval[a + self.m: a + lda] = 0.0
        return K


@pytest.mark.parametrize("regime", ["ones", "mid"])
@pytest.mark.parametrize("m,n", [(333, 1001), (800, 1600)])
def test_factorisation_schedule_on_the_cpu(m, n, regime):
    """The schedule the dense handle exports, executed in numpy on numpy's K: max|L - cholesky(K)| <= 1e-11 max|L|."""
    A = dense_A(m, n, seed=m)
    kkt = tk.setup(A, tk.K1(), tk.DenseBackend(device=-1))
    em = DenseEmulator(kkt)
    th, rp, rd, _, _ = ipm_like_data(m, n, 1, regime)
    K = em.update(th, rp, rd)
    L = em.dense_L()
    Lo = np.linalg.cholesky(K)
    err = np.abs(L - Lo).max() / np.abs(Lo).max()
    print(f"m={m} n={n} {regime}: max|L - L_numpy| / max|L| = {err:.2e}")
    assert np.isfinite(L).all() and err <= LTOL


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
def gpu_setup(A, **kw):
    return tk.setup(A, tk.K1(), tk.DenseBackend(device=0, **kw))


def check_factor_and_solution(A, kkt, regime, seed=3):
    m, n = A.shape
    th, rp, rd, xp, xd = ipm_like_data(m, n, seed, regime)
    tk.update(kkt, th, rp, rd)
    dx = np.zeros(n); dy = np.zeros(m)
    tk.solve(dx, dy, kkt, xp, xd)
    K, Lo, dxo, dyo = numpy_reference(A, th, rp, rd, xp, xd)
    L = panels_to_dense_L(kkt, kkt.factor_panels())
    el = np.abs(L - Lo).max() / np.abs(Lo).max()
    ey = np.abs(dy - dyo).max() / max(1.0, np.abs(dyo).max())
    ex = np.abs(dx - dxo).max() / max(1.0, np.abs(dxo).max())
    print(f"m={m} n={n} {regime}: L {el:.2e}  dy {ey:.2e}  dx {ex:.2e}")
    assert el <= LTOL and ey <= XTOL and ex <= XTOL
    return dx, dy


@pytest.mark.gpu
def test_dense_reference_conformance_routine():
    A = np.array([[1.0, 0, 1, 0], [0, 1, 0, 1]])
    kkt = gpu_setup(A)
    r1, r2 = tk.run_ls_tests(A, kkt)
    assert r1 <= SQRT_EPS and r2 <= SQRT_EPS
    assert tk.backend(kkt) == "HIP (gfx950)" and tk.linear_system(kkt) == "Normal equations (K1)"
    dx = np.zeros(4); dy = np.zeros(2)
    tk.solve(dx, dy, kkt, np.ones(2), np.ones(4))
    np.testing.assert_allclose(dy, [1.0, 1.0], atol=1e-15)
    np.testing.assert_allclose(dx, 0.0, atol=1e-15)


FACTOR_CASES = [(m, n, r) for (m, n) in [(1, 5), (256, 512), (333, 1001), (1000, 2000), (1500, 3000), (2049, 4100)] for r in ("ones", "mid")] + [(100, 37, "ones")]


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,regime", FACTOR_CASES)
def test_factor_and_solution_against_numpy(m, n, regime):
    A = dense_A(m, n, seed=m + n)
    check_factor_and_solution(A, gpu_setup(A), regime)


ILL_CASES = [(256, 512, "late"), (333, 1001, "late"), (1000, 2000, "late"), (2049, 4100, "late"), (100, 37, "mid")]


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,regime", ILL_CASES)
def test_ill_conditioned_residuals_against_numpy(m, n, regime):
    """No entrywise assertion (two CPU Choleskys with different summation orders differ by up to 1e-11 in L and 3e-8 in dy here):
    the update must succeed and the residuals of the Newton system stay within 10 x those of numpy's own factor."""
    A = dense_A(m, n, seed=m + n)
    th, rp, rd, xp, xd = ipm_like_data(m, n, 3, regime)
    kkt = gpu_setup(A)
    tk.update(kkt, th, rp, rd)
    dx = np.zeros(n); dy = np.zeros(m)
    tk.solve(dx, dy, kkt, xp, xd)
    _, _, dxo, dyo = numpy_reference(A, th, rp, rd, xp, xd)
    res = max(kkt_residuals(A, th, rp, rd, xp, xd, dx, dy))
    ref = max(kkt_residuals(A, th, rp, rd, xp, xd, dxo, dyo))
    print(f"m={m} n={n} {regime}: residual {res:.2e}, numpy's {ref:.2e}")
    assert np.isfinite(dx).all() and np.isfinite(dy).all() and res <= 10 * ref


@pytest.mark.gpu
def test_unwritten_panel_storage_is_never_read(monkeypatch):
    """k_zero_panels is not launched for dense handles: with the factor storage starting as NaNs the results must not change."""
    monkeypatch.setenv("TLPK_POISON", "1")
    for m, n in [(333, 1001), (1000, 2000)]:
        A = dense_A(m, n, seed=m + n)
        check_factor_and_solution(A, gpu_setup(A), "mid")


@pytest.mark.gpu
@pytest.mark.parametrize("m,n", [(333, 1001), (1500, 3000)])
def test_contracts_of_every_handle(m, n):
    A = dense_A(m, n, seed=5)
    th, rp, rd, xp, xd = ipm_like_data(m, n, 2, "mid")
    kkt = gpu_setup(A)
    # two updates with the same input: bit-identical panels
    tk.update(kkt, th, rp, rd); p0 = kkt.factor_panels().copy()
    tk.update(kkt, th, rp, rd); p1 = kkt.factor_panels().copy()
    assert np.array_equal(p0, p1, equal_nan=True)
    # host-pointer solve == device-pointer solve == each half of a pair, bit for bit
    dx = np.zeros(n); dy = np.zeros(m)
    tk.solve(dx, dy, kkt, xp, xd)
    xp1, xd1 = np.cos(np.arange(m, dtype=float)), np.sin(np.arange(n, dtype=float))
    dx1 = np.zeros(n); dy1 = np.zeros(m)
    tk.solve(dx1, dy1, kkt, xp1, xd1)
    b = {k: DevBuf(v) for k, v in dict(xp=xp, xd=xd, xp1=xp1, xd1=xd1).items()}
    o = {k: DevBuf(sz) for k, sz in dict(dx=n, dy=m, dx1=n, dy1=m, px=n, py=m, px1=n, py1=m).items()}
    kkt.solve_device(o["dx"].ptr, o["dy"].ptr, b["xp"].ptr, b["xd"].ptr)
    kkt.solve_device(o["dx1"].ptr, o["dy1"].ptr, b["xp1"].ptr, b["xd1"].ptr)
    kkt.solve2_device(o["px"].ptr, o["py"].ptr, b["xp"].ptr, b["xd"].ptr, o["px1"].ptr, o["py1"].ptr, b["xp1"].ptr, b["xd1"].ptr)
    assert np.array_equal(o["dx"].get(), dx) and np.array_equal(o["dy"].get(), dy)
    assert np.array_equal(o["dx1"].get(), dx1) and np.array_equal(o["dy1"].get(), dy1)
    assert np.array_equal(o["px"].get(), dx) and np.array_equal(o["py"].get(), dy)
    assert np.array_equal(o["px1"].get(), dx1) and np.array_equal(o["py1"].get(), dy1)
    # device-pointer update (and its asynchronous form, which may fall back to the blocking call) == host-pointer update
    d = {k: DevBuf(v) for k, v in dict(th=th, rp=rp, rd=rd).items()}
    kkt.update_device(d["th"].ptr, d["rp"].ptr, d["rd"].ptr)
    assert np.array_equal(kkt.factor_panels(), p0, equal_nan=True)
    kkt.update_device_async(d["th"].ptr, d["rp"].ptr, d["rd"].ptr); kkt.sync()
    assert np.array_equal(kkt.factor_panels(), p0, equal_nan=True)
    # a definitely indefinite matrix: PosDefException, and the handle stays usable
    D = 1.0 / (th + rp)
    lam = float(np.linalg.eigvalsh((A * D) @ A.T)[-1])
    with pytest.raises(tk.PosDefException):
        tk.update(kkt, th, rp, np.full(m, -2.0 * lam))
    assert kkt.stats()["fail_col"] >= 0
    check_factor_and_solution(A, kkt, "mid")
    # a view into a taller column-major array (lda > m) whose rows beyond m are NaN (a copy that read them would show): bit-identical to the packed copy
    big = np.full((m + 5, n), np.nan, order="F"); big[:m] = A
    kv = gpu_setup(big[:m])
    tk.update(kv, th, rp, rd)
    assert np.array_equal(kv.factor_panels(), p0, equal_nan=True)
    dxv = np.zeros(n); dyv = np.zeros(m)
    tk.solve(dxv, dyv, kv, xp, xd)
    assert np.array_equal(dxv, dx) and np.array_equal(dyv, dy)


@pytest.mark.gpu
def test_kernel_classes_of_a_profiled_step():
    m, n = 1500, 3000
    A = dense_A(m, n, seed=1)
    th, rp, rd, xp, xd = ipm_like_data(m, n, 0, "mid")
    kkt = gpu_setup(A, profile=True)
    tk.update(kkt, th, rp, rd)
    dx = np.zeros(n); dy = np.zeros(m)
    tk.solve(dx, dy, kkt, xp, xd)
    kt = kkt.kernel_times()
    print({k: (round(v["ms"], 4), v["launches"]) for k, v in kt.items()})
    assert kt["assemble"]["ms"] > 0 and kt["assemble"]["launches"] >= 2          # D, then the SYRK
    assert kt["spmv"]["ms"] > 0 and kt["spmv"]["launches"] >= 2                   # the two GEMVs
    assert kt["potrf"]["ms"] + kt["trsm"]["ms"] + kt["update"]["ms"] + kt["chain"]["ms"] > 0
    assert kt["solve_fwd"]["ms"] > 0 and kt["solve_bwd"]["ms"] > 0
    st = kkt.stats()
    assert st["device_bytes"] >= 8 * (m * n + m * (m + 1) // 2) and st["ms_last_update"] > 0
    kkt.set_profile(False)
    check_factor_and_solution(A, kkt, "mid")


def matrix_game():
    """max v : M'x - v 1 >= 0, 1'x = 1, x >= 0, v >= 0  (the value of the game is positive: v >= 0 is a valid bound)."""
    from tulip_jl_amd.problem import LP
    M = np.random.default_rng(7).uniform(0.0, 1.0, (120, 80))
    A = np.block([[M.T, -np.ones((80, 1))], [np.ones((1, 120)), np.zeros((1, 1))]])
    obj = np.zeros(121); obj[120] = 1.0
    lcon = np.concatenate([np.zeros(80), [1.0]]); ucon = np.concatenate([np.full(80, np.inf), [1.0]])
    return LP(A, obj, 0.0, lcon, ucon, np.zeros(121), np.full(121, np.inf), objsense_min=False, name="game"), A


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["hsd", "mpc"])
def test_matrix_game_end_to_end(algo):
    from scipy.optimize import linprog
    from tulip_jl_amd.hsd_device import DeviceHSD
    from tulip_jl_amd.mpc_device import DeviceMPC
    from tulip_jl_amd.problem import standard_form
    lp, A0 = matrix_game()
    d = standard_form(lp)
    assert d.A.shape == (81, 201)
    hs = linprog(-lp.obj, A_ub=-A0[:80], b_ub=np.zeros(80), A_eq=A0[80:], b_eq=[1.0], bounds=[(0, None)] * 121, method="highs")
    assert hs.status == 0
    zopt = -hs.fun
    cls = DeviceHSD if algo == "hsd" else DeviceMPC
    dense = cls(d.A.toarray(), d.b, d.c, d.l, d.u, c0=d.c0, objsense_min=d.objsense, dense=True, device=0).optimize()
    sparse = cls(d.A, d.b, d.c, d.l, d.u, c0=d.c0, objsense_min=d.objsense, device=0).optimize()
    sd, ss = dense.solution(nvar=d.nvar), sparse.solution(nvar=d.nvar)
    print(algo, "dense:", sd["status"], dense.niter, sd["z_primal"], sd["z_dual"], "| sparse:", ss["status"], sparse.niter, ss["z_primal"], ss["z_dual"], "| HiGHS:", zopt)
    assert isinstance(dense.kkt, tk.HIPDenseNormalEquations) and dense.kkt.stats()["n_pairs"] == 0
    assert sd["status"] == ss["status"] == "Trm_Optimal"
    assert abs(sd["z_primal"] - zopt) <= 1e-6 * (1 + abs(zopt))
    assert abs(dense.niter - sparse.niter) <= 1
    assert abs(sd["z_primal"] - ss["z_primal"]) <= 1e-8 * (1 + abs(ss["z_primal"]))
    assert abs(sd["z_dual"] - ss["z_dual"]) <= 1e-8 * (1 + abs(ss["z_dual"]))
