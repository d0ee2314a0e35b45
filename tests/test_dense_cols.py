"""K1 with dense columns as augmented nodes (tlpk_options.dense_cols): the columns of A with many entries stay out of A*D*A' and
become k extra nodes of the quasi-definite system [A_s D_s A_s' + Rd, A_d; A_d', -(Theta_d^-1 + Rp_d)] of order m + k, factorised by
the signed Cholesky of K2.  The caller still solves K1.  CPU: the column rule, the no-op guarantee, the refusals, the structure, the
rescue of an LP whose normal equations do not fit, and the signed schedule through the numpy emulator against the K1 oracle on the
FULL A.  GPU: the same against the HIP path, the bitwise contracts, refinement, the failure path and whole interior-point runs."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import tulip_jl_amd as tk
from tulip_jl_amd import _lib
from emulate import Emulator
from helpers import DevBuf, block_angular, ipm_like_data, kkt_residuals, random_lp_matrix
from oracle_binding import OracleK1


def k1(A, device=-1, **kw):
    return tk.setup(A, tk.K1(), tk.Backend(device=device, **kw))


def dense_of(kkt):
    return _lib.symbolic_array(kkt._h, "dense_cols")


def planted(m, n, nnz, counts, seed):
    """random_lp_matrix(m, n, nnz) plus one column per entry of `counts` with that many entries, the columns shuffled;
    returns (A, positions of the planted columns)."""
    A = random_lp_matrix(m, n, nnz, seed)
    rng = np.random.default_rng(seed + 7)
    extra = []
    for c in counts:
        rows = np.sort(rng.choice(m, size=c, replace=False))
        extra.append(sp.csc_matrix((rng.standard_normal(c), (rows, np.zeros(c, dtype=int))), shape=(m, 1)))
    B = sp.hstack([A] + extra, format="csc")
    p = rng.permutation(B.shape[1])
    B = B[:, p].tocsc()
    B.sort_indices()
    return B, np.argsort(p)[n:]


def chebyshev_matrix(q, p, seed, nnz_row=4):
    """Minimax (L-inf) regression rows |M beta - y| <= t in standard form: [M -e I 0; -M -e 0 I] (2q x (p + 1 + 2q));
    the t column touches every row.  M is banded (observation i sees features near i p / q): A_s A_s' fills little."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(q), nnz_row)
    cols = ((np.arange(q) * p) // q)[:, None].repeat(nnz_row, 1).ravel() + np.tile(np.arange(nnz_row), q)
    cols = cols % p
    M = sp.csr_matrix((rng.standard_normal(q * nnz_row), (rows, cols)), shape=(q, p))
    M.sum_duplicates()
    e = sp.csc_matrix(np.ones((q, 1)))
    I = sp.identity(q, format="csc")
    Z = sp.csc_matrix((q, q))
    A = sp.vstack([sp.hstack([M, -e, I, Z]), sp.hstack([-M, -e, Z, I])], format="csc")
    A.sort_indices()
    return A, M, rng


def two_stage_matrix(S=6, mk=60, nk=120, k1_=5, per=8, seed=0):
    """Dual block-angular: S scenario blocks W_s (mk x nk) and k1_ first-stage columns touching `per` rows of every scenario."""
    W = sp.block_diag([random_lp_matrix(mk, nk, 3, seed + s) for s in range(S)], format="csc")
    rng = np.random.default_rng(seed + 99)
    rows, cols = [], []
    for c in range(k1_):
        for s in range(S):
            r = s * mk + np.sort(rng.choice(mk, size=per, replace=False))
            rows.append(r); cols.append(np.full(per, c))
    rows = np.concatenate(rows); cols = np.concatenate(cols)
    T = sp.csc_matrix((rng.standard_normal(rows.size), (rows, cols)), shape=(S * mk, k1_))
    A = sp.hstack([T, W], format="csc")
    A.sort_indices()
    return A


class DenseEmulator(Emulator):
    """The device schedule of a handle with dense columns: D = [sparse j: 1 / (theta + regP), dense j: theta + regP ; 1], signs -1 on the
    dense nodes, right-hand side [xi_p + A_s D_s xi_d_s ; xi_d_d] permuted, output [dy ; dx_d] = P' x, dx_s = D_s (A_s' dy - xi_d_s)."""

    def __init__(self, kkt):
        super().__init__(kkt)
        self.dense = dense_of(kkt)
        self.sparse = np.ones(self.n, dtype=bool)
        self.sparse[self.dense] = False
        self.k2 = True                                    # the signed instances of the factor / sweep emulation
        self.sign = np.where(self.perm >= self.m, -1.0, 1.0)

    def update(self, theta, regP, regD, stop_at_marker=False):
        t = theta + regP
        self.Ds = np.where(self.sparse, 1.0 / t, 0.0)
        # the base class forms [theta + regP ; 1] for signed handles: hand it the D layout itself
        super().update(np.where(self.sparse, 1.0 / t, t), np.zeros_like(t), regD, stop_at_marker)

    def solve_local(self, xi_p, xi_d, A, rhs_rank=None):
        rhs = np.concatenate([xi_p + A @ (self.Ds * xi_d), xi_d[self.dense]])
        self.xw = rhs[self.perm].copy()
        for s_ in np.nonzero(self.single & (self.local != 0))[0]:
            l = self.Lval[self.loff[s_]]
            self.xw[self.col0[s_]] = self.xw[self.col0[s_]] / l / l
        self.ucflat = np.full(max(int((self.ucoff + self.f - self.ns).max()), 1), np.nan)
        self._resume_fwd = self._run(self.fwd_launches, True)

    def solve_finish(self, xi_d, A):
        self._run(self.fwd_launches, False, start=self._resume_fwd)
        self._bwd_seen = {}
        self.xw *= self.sign
        self._run(self.bwd_launches)
        sol = np.zeros(self.m + self.dense.size)
        sol[self.perm] = self.xw
        dy = sol[: self.m]
        dx = self.Ds * (A.T @ dy - xi_d)
        dx[self.dense] = sol[self.m:]
        return dx, dy


def close(a, b, tol=1e-9):
    return np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def test_rule_cap_and_flags():
    counts = [120, 80, 60, 150]
    A, where = planted(300, 600, 3, counts, seed=1)
    kkt = k1(A, dense_cols="auto", dense_col_min=50)
    assert dense_of(kkt).tolist() == sorted(where.tolist())
    assert kkt.stats()["n_dense_cols"] == 4 and kkt.stats()["m"] == 300 and kkt.stats()["n"] == A.shape[1]
    kkt = k1(A, dense_cols="auto", dense_col_min=50, max_dense_cols=2)            # the cap keeps the densest
    assert dense_of(kkt).tolist() == sorted(where[[3, 0]].tolist())
    assert kkt.stats()["n_dense_cols"] == 2
    kkt = k1(A, dense_cols="auto", dense_col_min=120)                              # MORE than dense_col_min entries
    assert dense_of(kkt).tolist() == [int(where[3])]
    kkt = k1(A, dense_cols=[5, 17], dense_col_min=500)                             # flags, whatever the count
    assert dense_of(kkt).tolist() == [5, 17] and kkt.stats()["n_dense_cols"] == 2
    assert tk.linear_system(kkt) == "Normal equations (K1)"


NOOP_ARRAYS = ["perm", "etree", "colcount", "s_colptr", "s_rowidx", "s_target", "s_diag_row", "pair_ptr", "pair_j", "rowidx", "rel",
               "front_f", "front_ns", "front_col0", "front_parent", "front_loff", "front_block", "front_group", "root_front", "row_block",
               "potrf_tasks", "trsm_tasks", "update_tasks", "ea_tasks", "fwd_sweep_tasks", "bwd_sweep_tasks", "factor_launches",
               "fwd_launches", "bwd_launches", "chain_items", "gth_src", "dense_cols"]


def raw_handle(A, **fields):
    """tlpk_create with explicitly set option fields (analyse only)."""
    L = _lib.lib()
    opt = _lib.Options()
    L.tlpk_default_options(C.byref(opt))
    opt.device = -1
    keep = []
    for k_, v in fields.items():
        if isinstance(v, np.ndarray):
            keep.append(v); v = _lib.as_p64(v)
        setattr(opt, k_, v)
    A = A.tocsc(); A.sort_indices()
    cp, rv, nz = (np.ascontiguousarray(A.indptr, dtype=np.int64), np.ascontiguousarray(A.indices, dtype=np.int64),
                  np.ascontiguousarray(A.data, dtype=np.float64))
    h = C.c_void_p()
    assert L.tlpk_create(C.byref(h), A.shape[0], A.shape[1], _lib.as_p64(cp), _lib.as_p64(rv), _lib.as_pd(nz), 0, C.byref(opt)) == _lib.OK
    return h


def snapshot(h):
    st = _lib.Stats()
    _lib.lib().tlpk_info(h, C.byref(st))
    d = {k_: v for k_, v in st.as_dict().items() if not k_.startswith("ms_")}
    for w in NOOP_ARRAYS:
        d[w] = _lib.symbolic_array(h, w).tolist()
    d["pair_w"] = _lib.symbolic_array_f64(h, "pair_w").tolist()
    return d


def noop_cases():
    import workloads
    from lp_generators import multicommodity_lp, staircase_lp
    A_ba, rb = block_angular(nblocks=4, mk=50, nk=110, m0=6, nnz_in=3, link_prob=0.5, seed=2)
    A_b0, rb0 = workloads.block_angular_lp(nblocks=4, mk=50, nk=110, m0=0, nnz_in=3, seed=4)
    W, rbw = workloads.block_angular_lp(nblocks=3, mk=80, nk=160, m0=10, nnz_in=4, seed=5)
    return [("random", random_lp_matrix(200, 500, 3, 2), {}),
            ("block_link", A_ba, {"row_block": rb}),
            ("block_nolink", A_b0, {"row_block": rb0}),
            ("block_detect", A_ba, {"detect_blocks": 1}),
            ("staircase", staircase_lp().A, {}),
            ("multicommodity", multicommodity_lp(nodes=120, K=3).A, {}),
            ("workloads_block", W, {"row_block": rbw}),
            ("workloads_general", workloads.general_sparse_lp(m=400, nnz_col=5), {})]


@pytest.mark.parametrize("case", range(8))
def test_no_dense_column_is_a_noop(case):
    name, A, kw = noop_cases()[case]
    ref = snapshot(raw_handle(A, **kw))
    assert ref["n_dense_cols"] == 0
    assert snapshot(raw_handle(A, dense_cols=0, **kw)) == ref, name          # explicit off
    assert snapshot(raw_handle(A, dense_cols=1, **kw)) == ref, name          # on, k == 0


def test_refusals():
    A, _ = planted(200, 400, 3, [90], seed=2)
    with pytest.raises(tk.DimensionMismatch, match="dense_cols"):
        tk.setup(A, tk.K2(), tk.Backend(device=-1, dense_cols="auto", dense_col_min=50))
    Ab, rb = block_angular(nblocks=4, mk=50, nk=110, m0=6, nnz_in=3, link_prob=0.5, seed=2)
    with pytest.raises(tk.DimensionMismatch, match="dense_cols"):
        tk.setup(Ab, tk.K1(), tk.Backend(device=-1, row_block=rb, rank=0, nranks=2, dense_cols="auto"))
    with pytest.raises(tk.DimensionMismatch, match="dense_cols"):
        tk.setup(Ab, tk.K1(), tk.Backend(row_block=rb, ngpus=2, devices=[0, 0], dense_cols="auto"))


def test_structure_general_and_block_path():
    m, counts = 400, [200, 150, 90]
    A, where = planted(m, 900, 3, counts, seed=3)
    k = len(counts)
    kkt = k1(A, dense_cols="auto", dense_col_min=50)
    perm = kkt.symbolic("perm")
    assert sorted(perm[-k:].tolist()) == list(range(m, m + k))                 # general path: the dense nodes last
    assert sorted(kkt.perm().tolist()) == list(range(m))                       # tlpk_get_perm: the constraint nodes
    As = A.tolil(); As[:, where] = 0.0
    As = As.tocsc(); As.eliminate_zeros()
    assert kkt.stats()["nnzL"] <= k1(As).stats()["nnzL"] + m * k + k * (k + 1) // 2
    # block path: the dense nodes join the linking rows in the root front
    Ab, rb = block_angular(nblocks=4, mk=80, nk=160, m0=8, nnz_in=3, link_prob=0.5, seed=5)
    mb = Ab.shape[0]
    rng = np.random.default_rng(5)
    D = sp.csc_matrix((rng.standard_normal(3 * 60), (np.concatenate([np.sort(rng.choice(mb, 60, replace=False)) for _ in range(3)]),
                                                      np.repeat(np.arange(3), 60))), shape=(mb, 3))
    Ab = sp.hstack([D, Ab], format="csc")
    kkt = k1(Ab, row_block=rb, dense_cols="auto", dense_col_min=40)
    st = kkt.stats()
    assert st["n_dense_cols"] == 3 and st["n_blocks"] == 4
    rf = int(kkt.symbolic("root_front")[0])
    c0, ns = int(kkt.symbolic("front_col0")[rf]), int(kkt.symbolic("front_ns")[rf])
    assert {mb, mb + 1, mb + 2} <= set(kkt.symbolic("perm")[c0: c0 + ns].tolist())


def test_two_stage_lp_detects_the_scenarios():
    A = two_stage_matrix(S=6)
    kkt = k1(A, row_block="auto", dense_cols=list(range(5)))
    st = kkt.stats()
    assert st["n_dense_cols"] == 5 and st["n_blocks"] == 6


def test_rescue_of_a_chebyshev_lp_whose_normal_equations_do_not_fit():
    """Fails at the parent commit: there is no dense_cols option, and plain K1 forms the dense 4000 x 4000 clique of the t column."""
    A, _, _ = chebyshev_matrix(2000, 2000, seed=1)
    plain = k1(A).stats()
    dense = k1(A, dense_cols="auto").stats()
    assert dense["n_dense_cols"] == 1 and dense["nnzL"] < 0.05 * plain["nnzL"]
    budget = int(8 * np.sqrt(plain["nnzL_stored"] * 4.0 * dense["nnzL_stored"]))
    with pytest.raises(tk.OutOfMemoryError):
        k1(A, mem_budget_bytes=budget)
    kkt = k1(A, mem_budget_bytes=budget, dense_cols="auto")
    assert kkt.stats()["nnzL"] == dense["nnzL"]


def emulated_case(m, n, k, seed, regime, relax, block=False):
    if block:
        A, rb = block_angular(nblocks=4, mk=m // 4, nk=n // 4, m0=6, nnz_in=3, link_prob=0.5, seed=seed)
        mm = A.shape[0]
        rng = np.random.default_rng(seed)
        cols = [sp.csc_matrix((rng.standard_normal(60), (np.sort(rng.choice(mm, 60, replace=False)), np.zeros(60, dtype=int))), shape=(mm, 1))
                for _ in range(k)]
        A = sp.hstack(cols + [A], format="csc")
        A.sort_indices()
        kw = {"row_block": rb}
    else:
        A, _ = planted(m, n, 3, [60 + (7 * t) % 90 for t in range(k)], seed)
        kw = {}
    kkt = k1(A, dense_cols="auto", dense_col_min=40, relax=relax, **kw)
    assert kkt.stats()["n_dense_cols"] == k
    th, rp, rd, xp, xd = ipm_like_data(A.shape[0], A.shape[1], seed, regime)
    return A, kkt, (th, rp, rd, xp, xd)


@pytest.mark.parametrize("k", [1, 7, 40])
@pytest.mark.parametrize("regime", ["mid", "late"])
@pytest.mark.parametrize("relax", [0, 1])
def test_emulated_schedule_vs_k1_oracle(k, regime, relax):
    A, kkt, (th, rp, rd, xp, xd) = emulated_case(300, 700, k, 10 + k, regime, relax)
    em = DenseEmulator(kkt)
    em.update(th, rp, rd)
    assert em.fail_col is None
    dx, dy = em.solve(xp, xd, A)
    check_vs_oracle(A, (th, rp, rd, xp, xd), dx, dy, regime)


def check_vs_oracle(A, data, dx, dy, regime):
    """The K1 oracle forms the dense A D A' of the FULL A.  "mid": solutions to 1e-9, residuals <= 1e-8 (1 + |xi|).  "late" (cond(S) near
    1 / eps): plain K1's own residuals are ~1e-6 there, so the solution is held to residuals no worse than 10 x the oracle's."""
    th, rp, rd, xp, xd = data
    orc = OracleK1(A); orc.update(th, rp, rd)
    dxo, dyo = orc.solve(xp, xd)
    r = max(kkt_residuals(A, th, rp, rd, xp, xd, dx, dy))
    bound = 1e-8 * (1 + max(np.abs(xp).max(), np.abs(xd).max()))
    if regime == "mid":
        assert close(dx, dxo) and close(dy, dyo)
        assert r <= bound
    else:
        assert r <= max(bound, 10 * max(kkt_residuals(A, th, rp, rd, xp, xd, dxo, dyo)))


def test_emulated_block_path_vs_k1_oracle():
    A, kkt, (th, rp, rd, xp, xd) = emulated_case(320, 640, 3, 21, "mid", 1, block=True)
    em = DenseEmulator(kkt)
    em.update(th, rp, rd)
    dx, dy = em.solve(xp, xd, A)
    orc = OracleK1(A); orc.update(th, rp, rd)
    dxo, dyo = orc.solve(xp, xd)
    assert close(dx, dxo) and close(dy, dyo)


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def gpu_solve(kkt, th, rp, rd, xp, xd):
    tk.update(kkt, th, rp, rd)
    dx = np.zeros(kkt.n); dy = np.zeros(kkt.m)
    tk.solve(dx, dy, kkt, xp, xd)
    return dx, dy


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(300, 700, 1, False), (300, 700, 40, False), (1500, 3500, 7, False), (3000, 7000, 12, False), (1200, 2400, 5, True)])
@pytest.mark.parametrize("regime", ["mid", "late"])
def test_gpu_parity_vs_k1_oracle(case, regime):
    m, n, k, block = case
    A, kkt0, (th, rp, rd, xp, xd) = emulated_case(m, n, k, 30 + k, regime, 1, block=block)
    kw = {"row_block": kkt0.backend_options.row_block} if block else {}
    kkt = k1(A, device=0, dense_cols="auto", dense_col_min=40, **kw)
    dx, dy = gpu_solve(kkt, th, rp, rd, xp, xd)
    check_vs_oracle(A, (th, rp, rd, xp, xd), dx, dy, regime)


@pytest.mark.gpu
def test_gpu_bitwise_contracts():
    A, where = planted(800, 1800, 3, [300, 120, 200], seed=44)
    m, n = A.shape
    th, rp, rd, xp, xd = ipm_like_data(m, n, 44)
    xp1, xd1 = np.random.default_rng(45).standard_normal(m), np.random.default_rng(46).standard_normal(n)
    kkt = k1(A, device=0, dense_cols="auto", dense_col_min=100)
    d = [DevBuf(v) for v in (th, rp, rd, xp, xd, xp1, xd1)]
    kkt.update_device(d[0].ptr, d[1].ptr, d[2].ptr)
    o = [DevBuf(sz) for sz in (n, m, n, m, n, m, n, m)]
    kkt.solve_device(o[0].ptr, o[1].ptr, d[3].ptr, d[4].ptr)
    kkt.solve_device(o[2].ptr, o[3].ptr, d[5].ptr, d[6].ptr)
    kkt.solve2_device(o[4].ptr, o[5].ptr, d[3].ptr, d[4].ptr, o[6].ptr, o[7].ptr, d[5].ptr, d[6].ptr)
    single = [b.get() for b in o[:4]]
    pair = [b.get() for b in o[4:]]
    for a_, b_ in zip(single, pair):
        assert np.array_equal(a_, b_)                                          # pair == two single solves
    dx, dy = gpu_solve(kkt, th, rp, rd, xp, xd)                                # host-pointer path == device-pointer path
    assert np.array_equal(dx, single[0]) and np.array_equal(dy, single[1])
    kkt2 = k1(A, device=0, dense_cols="auto", dense_col_min=100)               # a second handle
    dx2, dy2 = gpu_solve(kkt2, th, rp, rd, xp, xd)
    assert np.array_equal(dx2, dx) and np.array_equal(dy2, dy)
    kkt3 = k1(A, device=0, dense_cols=sorted(where.tolist()), dense_col_min=10 ** 6)    # the same columns by flag
    assert dense_of(kkt3).tolist() == dense_of(kkt).tolist()
    dx3, dy3 = gpu_solve(kkt3, th, rp, rd, xp, xd)
    assert np.array_equal(dx3, dx) and np.array_equal(dy3, dy)


@pytest.mark.gpu
def test_gpu_rescue_and_agreement_with_plain_k1():
    A, _, _ = chebyshev_matrix(2000, 2000, seed=1)
    m, n = A.shape
    th, rp, rd, xp, xd = ipm_like_data(m, n, 3, "mid")
    plain_host = k1(A).stats(); dense_host = k1(A, dense_cols="auto").stats()
    budget = int(8 * np.sqrt(plain_host["nnzL_stored"] * 4.0 * dense_host["nnzL_stored"]))
    with pytest.raises(tk.OutOfMemoryError, match="does not form A.D.A'; or keep K1 with dense_cols = 1"):
        k1(A, device=0, mem_budget_bytes=budget)                               # the hint names both ways out
    kkt = k1(A, device=0, mem_budget_bytes=budget, dense_cols="auto")
    dx, dy = gpu_solve(kkt, th, rp, rd, xp, xd)
    r1, r2 = kkt_residuals(A, th, rp, rd, xp, xd, dx, dy)
    assert max(r1, r2) <= 1e-8 * (1 + max(np.abs(xp).max(), np.abs(xd).max()))
    dxp, dyp = gpu_solve(k1(A, device=0), th, rp, rd, xp, xd)                  # plain K1 without the budget
    assert close(dx, dxp) and close(dy, dyp)


@pytest.mark.gpu
def test_gpu_refinement_on_a_dense_handle():
    A, _ = planted(1000, 2200, 3, [400, 250], seed=7)
    m, n = A.shape
    th, rp, rd, xp, xd = ipm_like_data(m, n, 7, "late")
    res = []
    for refine in (0, 1):
        kkt = k1(A, device=0, dense_cols="auto", dense_col_min=100, refine=refine)
        dx, dy = gpu_solve(kkt, th, rp, rd, xp, xd)
        res.append(max(kkt_residuals(A, th, rp, rd, xp, xd, dx, dy)))
        assert kkt.stats()["refine_rejected"] >= 0
    assert res[1] <= res[0] * (1 + 1e-12) + 1e-300


@pytest.mark.gpu
def test_gpu_wrong_sign_pivot_is_reported_and_the_handle_recovers():
    A, where = planted(400, 800, 3, [150], seed=9)
    A = A.tolil()
    r = int(np.flatnonzero(A[:, int(where[0])].toarray().ravel())[0])
    for j in range(A.shape[1]):                         # row r: touched by the dense column only, so A_s is rank deficient
        if j != int(where[0]):
            A[r, j] = 0.0
    A = A.tocsc(); A.eliminate_zeros()
    m, n = A.shape
    th, rp, rd, xp, xd = ipm_like_data(m, n, 9, "mid")
    kkt = k1(A, device=0, dense_cols="auto", dense_col_min=100)
    with pytest.raises(tk.PosDefException):
        tk.update(kkt, th, rp, np.zeros(m))
    dx, dy = gpu_solve(kkt, th, rp, rd, xp, xd)
    r1, r2 = kkt_residuals(A, th, rp, rd, xp, xd, dx, dy)
    assert max(r1, r2) <= 1e-8 * (1 + max(np.abs(xp).max(), np.abs(xd).max()))


def planted_lp(A, seed):
    """A feasible, bounded LP on A: a planted interior point and box bounds."""
    m, n = A.shape
    rng = np.random.default_rng(seed)
    xs = rng.uniform(0.2, 1.0, n)
    b = A @ xs
    c = rng.standard_normal(n)
    return b, c, np.zeros(n), np.full(n, 2.0)


def highs_opt(A, b, c, l, u):
    from scipy.optimize import linprog
    r = linprog(c, A_eq=A, b_eq=b, bounds=list(zip(l, u)), method="highs")
    assert r.status == 0, r.message
    return r.fun


@pytest.mark.gpu
@pytest.mark.parametrize("lp", ["chebyshev", "two_stage"])
def test_gpu_device_hsd_dense_cols_vs_k2(lp):
    from tulip_jl_amd.hsd_device import DeviceHSD
    if lp == "chebyshev":
        A, _, _ = chebyshev_matrix(600, 300, seed=4)
        kw = {"dense_cols": "auto", "dense_col_min": 500}
    else:
        A = two_stage_matrix(S=5, mk=50, nk=100, k1_=4, per=6, seed=3)
        kw = {"dense_cols": list(range(4)), "row_block": "auto"}
    b, c, l, u = planted_lp(A, 11)
    sols = []
    for system, extra in (("K1", kw), ("K2", {"row_block": "auto"} if lp == "two_stage" else {})):
        opt = DeviceHSD(A, b, c, l, u, system=system, device=0, **extra)
        if system == "K1":
            assert opt.kkt.stats()["n_dense_cols"] >= 1
        opt.optimize()
        sols.append((opt, opt.solution()))
    (h1, s1), (h2, s2) = sols
    assert s1["status"] == s2["status"] == "Trm_Optimal"
    assert abs(h1.niter - h2.niter) <= 1
    assert abs(s1["z_primal"] - s2["z_primal"]) <= 1e-8 * (1 + abs(s2["z_primal"]))
    ref = highs_opt(A, b, c, l, u)
    assert abs(s1["z_primal"] - ref) <= 1e-6 * (1 + abs(ref))
