"""tlpk_set_values* / tlpk_ipm_reload: new numerical values on an analysed pattern.

The analysis does not depend on the values (explicit zeros included), so the acceptance criterion is BITWISE equality with a fresh
handle created on the new values: the symbolic arrays are unchanged, the products of the assembly lists, the factor and the
solutions carry the same bits.  In every test the second value set is standard-normal with every 17th entry an exact 0.0 and signs
independent of the first set."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import tulip_jl_amd as tk
from emulate import Emulator, unpack_panel
from helpers import DevBuf, block_angular, ipm_like_data, random_lp_matrix
from oracle_binding import OracleK1
from tulip_jl_amd import _lib

NEW = ["tlpk_set_values", "tlpk_set_values_device", "tlpk_set_values_dense", "tlpk_set_values_dense_device", "tlpk_ipm_reload"]
# what the analysis produces, as far as tlpk_symbolic_get exports it
SYMBOLIC = ["perm", "etree", "colcount", "s_colptr", "s_rowidx", "s_target", "s_diag_row", "pair_ptr", "pair_j", "rowidx", "rel",
            "front_f", "front_ns", "front_col0", "front_lda", "front_loff", "front_parent", "gth_ptr", "gth_src", "update_tasks", "potrf_tasks",
            "trsm_tasks", "upd_seg", "factor_launches", "fwd_launches", "bwd_launches", "row_block", "front_block", "front_local", "dense_cols"]


def second_values(count, seed=4242):
    v = np.random.default_rng(seed).standard_normal(count)
    v[::17] = 0.0
    return v


def with_values(A, nz):
    return sp.csc_matrix((np.asarray(nz, dtype=float).copy(), A.indices.copy(), A.indptr.copy()), shape=A.shape)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def dense_cols_matrix(seed=5):
    A, rb = block_angular(4, 150, 300, 20, 3, 0.3, seed)
    rng = np.random.default_rng(seed + 1)
    D = sp.random(A.shape[0], 3, density=0.6, random_state=seed + 2, format="csc", data_rvs=rng.standard_normal)
    B = sp.hstack([A, D], format="csc")
    B.sort_indices()
    return B, rb


def cases():
    """name -> (A, system, backend keywords without the device)"""
    G = random_lp_matrix(300, 700, 4, 1)
    B, rb = block_angular(4, 150, 300, 20, 3, 0.3, 5)
    Bd, _ = dense_cols_matrix()
    return {
        "k1_general": (G, tk.K1(), {}),
        "k2_general": (G, tk.K2(), {}),
        "k1_block": (B, tk.K1(), dict(row_block=rb)),
        "k2_block": (B, tk.K2(), dict(row_block=rb)),
        "k1_rank1of2": (B, tk.K1(), dict(row_block=rb, rank=1, nranks=2)),
        "k2_rank1of2": (B, tk.K2(), dict(row_block=rb, rank=1, nranks=2)),
        "k1_dense_cols": (Bd, tk.K1(), dict(dense_cols="auto", dense_col_min=100)),
    }


CASES = cases()


class DenseColsEmulator(Emulator):
    """The schedule of a handle with dense columns (include/tlpk.h, tlpk_options.dense_cols): D = [sparse j: 1 / (theta + regP), dense j:
    theta + regP ; 1], signs -1 on the dense nodes, right-hand side [xi_p + A_s D_s xi_d_s ; xi_d_d], output [dy ; dx_d]."""

    def __init__(self, kkt):
        super().__init__(kkt)
        self.dense = kkt.symbolic("dense_cols")
        self.sparse = np.ones(self.n, dtype=bool)
        self.sparse[self.dense] = False
        self.k2 = True
        self.sign = np.where(self.perm >= self.m, -1.0, 1.0)

    def update(self, theta, regP, regD, stop_at_marker=False):
        t = theta + regP
        self.Ds = np.where(self.sparse, 1.0 / t, 0.0)
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


def emulate(kkt, A, data, sharded):
    """Factor (and, on a whole handle, the solution) of the numpy emulation of the handle's schedule; it reads pair_w from the handle."""
    th, rp, rd, xp, xd = data
    em = (DenseColsEmulator if kkt.stats()["n_dense_cols"] else Emulator)(kkt)
    em.update(th, rp, rd, stop_at_marker=sharded)          # a rank of a sharded job: everything up to the reduction of the root panel
    out = [em.Lval.copy()] + [em.panel(s).copy() for s in range(len(em.f)) if em.local[s] and not em.single[s]]
    if not sharded:
        assert em.fail_col is None
        out += list(em.solve(xp, xd, A))
    return out


# ---------------------------------------------------------------------------------------------
# CPU: analyse-only handles, the host path
# ---------------------------------------------------------------------------------------------
def test_abi_declares_exports_and_mirrors_the_new_entry_points():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tlpk.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert f"int {name}(tlpk_handle *h" in hdr, name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    fields = [f for f, _ in _lib.Stats._fields_]
    assert fields[-2:] == ["ms_last_set_values", "set_values_bytes"]
    # every field of tlpk_stats is 8 bytes except the pair of int32: the mirror's size is the header's
    body = hdr[hdr.index("typedef struct tlpk_stats {") + len("typedef struct tlpk_stats {"): hdr.index("} tlpk_stats;")]
    import re
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    n64 = n32 = 0
    for decl in body.split(";"):
        decl = decl.strip()
        if decl.startswith(("int64_t", "double")):
            n64 += decl.count(",") + 1
        elif decl.startswith("int32_t"):
            n32 += decl.count(",") + 1
    assert C.sizeof(_lib.Stats) == 8 * n64 + 4 * n32
    assert n64 + n32 == len(fields)


@pytest.mark.parametrize("name", list(CASES))
def test_host_refresh_equals_a_fresh_handle_bitwise(name):
    A, system, kw = CASES[name]
    sharded = kw.get("nranks", 1) > 1
    nz1, nz2 = A.data.copy(), second_values(A.nnz)
    A2 = with_values(A, nz2)
    kkt = tk.setup(A, system, tk.Backend(device=-1, **kw))
    sym1 = {w: kkt.symbolic(w).copy() for w in SYMBOLIC}
    w1 = _lib.symbolic_array_f64(kkt._h, "pair_w").copy()
    ms_analyse = kkt.stats()["ms_analyse"]
    tk.set_values(kkt, nz2)
    assert same_bits(kkt.A.data, nz2) and kkt.A.shape == A.shape
    fresh = tk.setup(A2, system, tk.Backend(device=-1, **kw))
    for w in SYMBOLIC:
        assert np.array_equal(kkt.symbolic(w), sym1[w]), w                   # nothing of the analysis moved ...
        assert np.array_equal(fresh.symbolic(w), sym1[w]), w                 # ... and it does not depend on the values
    w2 = _lib.symbolic_array_f64(kkt._h, "pair_w").copy()
    assert len(w2) == kkt.stats()["n_pairs"] > 0
    assert same_bits(w2, _lib.symbolic_array_f64(fresh._h, "pair_w"))
    assert not same_bits(w2, w1)
    st = kkt.stats()
    assert st["ms_analyse"] == ms_analyse and st["ms_last_set_values"] > 0 and st["set_values_bytes"] == 0
    data = ipm_like_data(A.shape[0], A.shape[1], 3)
    got, want = emulate(kkt, A2, data, sharded), emulate(fresh, A2, data, sharded)
    assert len(got) == len(want) and all(same_bits(a, b) for a, b in zip(got, want))
    if not sharded and isinstance(system, tk.K1):
        # the refreshed handle solves the NEW system: the K1 oracle on nz2, at the factor / solution tolerances of tests/test_gpu_parity.py
        th, rp, rd, xp, xd = data
        orc = OracleK1(A2) if kw.get("dense_cols") else OracleK1(A2, kkt.perm())
        orc.update(th, rp, rd)
        dxo, dyo = orc.solve(xp, xd)
        dx, dy = got[-2], got[-1]
        assert np.abs(dy - dyo).max() <= 1e-9 * max(1.0, np.abs(dyo).max())
        assert np.abs(dx - dxo).max() <= 1e-9 * max(1.0, np.abs(dxo).max())
        if not kw.get("dense_cols"):
            em = Emulator(kkt); em.update(th, rp, rd)
            Lo = orc.get_L().toarray()
            assert np.abs(em.dense_L() - Lo).max() <= 1e-11 * np.abs(Lo).max()
    # round trip: the first values again give the first products, bit for bit
    tk.set_values(kkt, with_values(A, nz1))
    assert same_bits(_lib.symbolic_array_f64(kkt._h, "pair_w"), w1)


def test_refusals_leave_the_handle_untouched():
    L = _lib.lib()
    A = random_lp_matrix(60, 140, 3, 2)
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=-1))
    w1 = _lib.symbolic_array_f64(kkt._h, "pair_w").copy()
    nz2 = second_values(A.nnz)
    assert L.tlpk_set_values(kkt._h, None, A.nnz) == _lib.BADARG and b"NULL" in L.tlpk_last_error(kkt._h)
    assert L.tlpk_set_values(kkt._h, _lib.as_pd(nz2), A.nnz - 1) == _lib.BADARG and b"len" in L.tlpk_last_error(kkt._h)
    assert L.tlpk_set_values(kkt._h, _lib.as_pd(nz2), A.nnz + 1) == _lib.BADARG
    assert L.tlpk_set_values(None, _lib.as_pd(nz2), A.nnz) == _lib.BADARG
    D = np.asfortranarray(np.ones((60, 140)))
    assert L.tlpk_set_values_dense(kkt._h, D.ctypes.data_as(_lib.pd), 60) == _lib.BADARG and b"dense" in L.tlpk_last_error(kkt._h)
    assert same_bits(_lib.symbolic_array_f64(kkt._h, "pair_w"), w1)
    assert L.tlpk_set_values_device(kkt._h, 1 << 20, A.nnz) == _lib.NO_DEVICE          # analyse-only: the pointer is never touched
    assert L.tlpk_ipm_reload(kkt._h, None, None, None, None) == _lib.NO_DEVICE
    with pytest.raises(tk.DimensionMismatch):
        tk.set_values(kkt, random_lp_matrix(60, 140, 3, 3))                             # another pattern
    with pytest.raises(tk.DimensionMismatch):
        tk.set_values(kkt, nz2[:-1])
    assert same_bits(_lib.symbolic_array_f64(kkt._h, "pair_w"), w1)
    dk = tk.setup(np.ones((7, 9)), tk.K1(), tk.DenseBackend(device=-1))
    assert L.tlpk_set_values(dk._h, _lib.as_pd(nz2), 63) == _lib.BADARG and b"tlpk_set_values_dense" in L.tlpk_last_error(dk._h)
    E = np.asfortranarray(np.ones((7, 9)))
    assert L.tlpk_set_values_dense(dk._h, E.ctypes.data_as(_lib.pd), 6) == _lib.BADARG and b"lda" in L.tlpk_last_error(dk._h)
    assert L.tlpk_set_values_dense(dk._h, None, 7) == _lib.BADARG
    assert L.tlpk_set_values_dense_device(dk._h, 1 << 20, 7) == _lib.NO_DEVICE
    assert L.tlpk_set_values_dense(dk._h, E.ctypes.data_as(_lib.pd), 7) == _lib.OK
    with pytest.raises(tk.DimensionMismatch):
        tk.set_values(dk, np.ones((7, 8)))


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def results(kkt, data, factor=True):
    """update, the factor panels, one solve (host pointers) and a pair (device pointers) whose first system is that solve"""
    th, rp, rd, xp, xd = data
    m, n = kkt.m, kkt.n
    tk.update(kkt, th, rp, rd)
    out = [factor_entries(kkt, kkt.factor_panels())] if factor else []
    dx = np.zeros(n); dy = np.zeros(m)
    tk.solve(dx, dy, kkt, xp, xd)
    out += [dx, dy]
    if factor:                                                                # (single-device handles: the device-pointer entry points)
        d = [DevBuf(v) for v in (xp, xd, xp[::-1].copy(), xd[::-1].copy())]
        o = [DevBuf(sz, 0.0) for sz in (n, m, n, m)]
        kkt.solve2_device(o[0].ptr, o[1].ptr, d[0].ptr, d[1].ptr, o[2].ptr, o[3].ptr, d[2].ptr, d[3].ptr)
        out += [b.get() for b in o]
    return out


def all_same(a, b):
    return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))


def factor_entries(kkt, lval):
    """The entries of L in the panel storage tlpk_get_factor copies: per local front the lower trapezoid of its f x ns panel.  The rest of the
    storage -- the strict upper triangles of the diagonal blocks, the padding rows up to the leading dimension -- is scratch that no kernel
    reads as part of L and that the zero-fill may skip: it is not compared."""
    g = kkt.symbolic
    f, ns, loff, lda, local = g("front_f"), g("front_ns"), g("front_loff"), g("front_lda"), g("front_local")
    out = []
    for s in range(len(f)):
        if not local[s]:
            continue
        P = unpack_panel(lval, int(loff[s]), int(f[s]), int(ns[s]), int(lda[s]))
        out.append(P[np.tril_indices(int(f[s]), 0, int(ns[s]))])
    return np.concatenate(out) if out else np.zeros(0)


def not_factored(kkt):
    dx = np.zeros(kkt.n); dy = np.zeros(kkt.m)
    return _lib.lib().tlpk_solve(kkt._h, _lib.as_pd(dx), _lib.as_pd(dy), _lib.as_pd(np.ones(kkt.m)), _lib.as_pd(np.ones(kkt.n))) == _lib.NOT_FACTORED


GPU_CASES = {
    "k1_general": CASES["k1_general"], "k1_block": CASES["k1_block"], "k2_general": CASES["k2_general"], "k2_block": CASES["k2_block"],
    "k1_dense_cols": CASES["k1_dense_cols"], "k1_refine": (CASES["k1_general"][0], tk.K1(), dict(refine=1)),
    "k1_blocked_front": (random_lp_matrix(1200, 3000, 4, 7), tk.K1(), {}),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GPU_CASES))
def test_gpu_refresh_equals_a_fresh_handle_bitwise(name):
    A, system, kw = GPU_CASES[name]
    if name == "k1_blocked_front":
        assert tk.setup(A, system, tk.Backend(device=-1)).stats()["max_front"] > 256       # the blocked factorisation
    nz1, nz2 = A.data.copy(), second_values(A.nnz)
    A2 = with_values(A, nz2)
    data = ipm_like_data(A.shape[0], A.shape[1], 3)
    kkt = tk.setup(A, system, tk.Backend(device=0, **kw))
    bytes0 = kkt.stats()["device_bytes"]
    assert kkt.stats()["set_values_bytes"] == 0
    first = results(kkt, data)
    tk.set_values(kkt, nz2)
    assert not_factored(kkt)
    st = kkt.stats()
    assert st["set_values_bytes"] > 0 and st["device_bytes"] == bytes0 + st["set_values_bytes"] and st["ms_last_set_values"] > 0
    second = results(kkt, data)
    fresh = tk.setup(A2, system, tk.Backend(device=0, **kw))
    want = results(fresh, data)
    assert fresh.stats()["device_bytes"] == bytes0 and fresh.stats()["set_values_bytes"] == 0     # a handle that never calls it pays nothing
    assert all_same(second, want)
    assert not all_same(second, first)
    assert same_bits(_lib.symbolic_array_f64(kkt._h, "pair_w"), _lib.symbolic_array_f64(tk.setup(A2, system, tk.Backend(device=-1, **kw))._h, "pair_w"))
    tk.run_ls_tests(A2, kkt)
    # the first values again: the first results, bit for bit; and no further growth of the handle
    tk.set_values(kkt, with_values(A, nz1))
    assert all_same(results(kkt, data), first)
    # the device-pointer variant gives the bits of the host variant
    buf = DevBuf(nz2)
    tk.set_values_device(kkt, buf.ptr, A.nnz)
    assert not_factored(kkt)
    kkt.sync()
    assert all_same(results(kkt, data), want)
    for _ in range(2):
        tk.set_values(kkt, nz1)
        assert kkt.stats()["device_bytes"] == st["device_bytes"]
    L = _lib.lib()
    assert L.tlpk_set_values(kkt._h, _lib.as_pd(nz2), A.nnz - 1) == _lib.BADARG
    tk.update(kkt, *data[:3])
    assert L.tlpk_set_values(kkt._h, None, A.nnz) == _lib.BADARG and not not_factored(kkt)      # a refused call leaves the handle factored


@pytest.mark.gpu
def test_gpu_dense_matrix_handle():
    m, n = 200, 500                                                            # m is no multiple of 16: the padding rows of the device copy matter
    rng = np.random.default_rng(8)
    A1 = np.asfortranarray(rng.standard_normal((m, n)))
    A2 = np.asfortranarray(second_values(m * n).reshape((m, n), order="F"))
    data = ipm_like_data(m, n, 3)
    kkt = tk.setup(A1, tk.K1(), tk.DenseBackend(device=0))
    bytes0 = kkt.stats()["device_bytes"]
    first = results(kkt, data)
    tk.set_values(kkt, A2)                                                     # lda = m
    assert not_factored(kkt)
    second = results(kkt, data)
    want = results(tk.setup(A2, tk.K1(), tk.DenseBackend(device=0)), data)
    assert all_same(second, want) and not all_same(second, first)
    tk.run_ls_tests(A2, kkt)
    tk.set_values(kkt, A1)
    assert all_same(results(kkt, data), first)
    wide = np.full((m + 3, n), np.nan, order="F")                              # lda = m + 3: the rows beyond m are never read
    wide[:m] = A2
    L = _lib.lib()
    assert L.tlpk_set_values_dense(kkt._h, wide.ctypes.data_as(_lib.pd), m + 3) == _lib.OK
    assert all_same(results(kkt, data), want)
    tk.set_values(kkt, A1)
    buf = DevBuf(wide.reshape(-1, order="F"))
    assert L.tlpk_set_values_dense_device(kkt._h, buf.ptr, m + 3) == _lib.OK
    assert not_factored(kkt)
    kkt.sync()
    assert all_same(results(kkt, data), want)
    assert kkt.stats()["device_bytes"] == bytes0 and kkt.stats()["set_values_bytes"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("system", ["K1", "K2"])
def test_gpu_multi_device_handle(system):
    A, _, kw = CASES["k1_block"]
    sysobj = tk.K1() if system == "K1" else tk.K2()
    nz2 = second_values(A.nnz)
    A2 = with_values(A, nz2)
    data = ipm_like_data(A.shape[0], A.shape[1], 3)
    be = dict(ngpus=2, devices=[0, 0], **kw)
    kkt = tk.setup(A, sysobj, tk.Backend(**be))
    first = results(kkt, data, factor=False)
    tk.set_values(kkt, nz2)                                                    # one call: the library serves both shards
    assert not_factored(kkt)
    bytes1 = kkt.stats()["device_bytes"]
    assert kkt.stats()["set_values_bytes"] > 0
    second = results(kkt, data, factor=False)
    want = results(tk.setup(A2, sysobj, tk.Backend(**be)), data, factor=False)
    assert all_same(second, want) and not all_same(second, first)
    tk.set_values(kkt, A)
    assert all_same(results(kkt, data, factor=False), first)
    assert kkt.stats()["device_bytes"] == bytes1
    assert _lib.lib().tlpk_set_values_device(kkt._h, 1 << 20, A.nnz) == _lib.BADARG


def sharded_step(ks, data):
    """One update + solve of a two-rank sharded job inside this process: the split-phase calls, the two reductions done here (sum in rank order)."""
    th, rp, rd, xp, xd = data
    m, n = ks[0].m, ks[0].n
    d = [DevBuf(v) for v in (th, rp, rd, xp, xd)]

    def reduce(which, count):
        bufs = [DevBuf(count, 0.0) for _ in ks]
        for k, b in zip(ks, bufs):
            k.root_copy(which, "out", b.ptr); k.sync()
        total = bufs[0].get()
        for b in bufs[1:]:
            total = total + b.get()
        t = DevBuf(total)
        for k in ks:
            k.root_copy(which, "in", t.ptr); k.sync()
        return total

    for k in ks:
        k.update_local(d[0].ptr, d[1].ptr, d[2].ptr); k.sync()
    panel = reduce("panel", ks[0].root_panel()[1])
    for k in ks:
        k.update_finish()
    for k in ks:
        k.solve_local(d[3].ptr, d[4].ptr); k.sync()
    reduce("rhs", ks[0].root_rhs()[1])
    out = [panel]
    for k in ks:
        o = [DevBuf(n, 0.0), DevBuf(m, 0.0)]
        k.solve_finish(o[0].ptr, o[1].ptr, d[4].ptr); k.sync()
        out += [o[0].get(), o[1].get(), factor_entries(k, k.factor_panels())]
    return out


@pytest.mark.gpu
def test_gpu_sharded_pair_in_one_process():
    A, _, kw = CASES["k1_block"]
    nz2 = second_values(A.nnz)
    A2 = with_values(A, nz2)
    data = ipm_like_data(A.shape[0], A.shape[1], 3)
    mk = lambda M: [tk.setup(M, tk.K1(), tk.Backend(device=0, rank=r, nranks=2, **kw)) for r in range(2)]      # noqa: E731
    ks = mk(A)
    first = sharded_step(ks, data)
    for k in ks:
        tk.set_values(k, nz2)                                                  # every rank passes the full nzval, as at create
    second = sharded_step(ks, data)
    want = sharded_step(mk(A2), data)
    assert all_same(second, want) and not all_same(second, first)
    for k in ks:
        tk.set_values(k, A)
    assert all_same(sharded_step(ks, data), first)


def block_angular_lp(seed=7):
    """A feasible, bounded LP on a 7-block block-angular matrix with a known optimal vertex; LP2 on the same pattern: A2 = R A for a positive
    diagonal R, b2 = R b, a new c, some lower bounds 0 -> -inf and some upper bounds +inf -> finite (the vertex stays optimal)."""
    A, rb = block_angular(nblocks=7, mk=120, nk=260, m0=30, nnz_in=3, link_prob=0.5, seed=seed)
    m, n = A.shape
    rng = np.random.default_rng(seed)
    xs = rng.uniform(0.0, 1.0, n) * (rng.random(n) < 0.6)
    ys = rng.standard_normal(m)
    zs = rng.uniform(0.0, 1.0, n) * (xs == 0.0)
    lp1 = (A, A @ xs, A.T @ ys + zs, np.zeros(n), np.full(n, np.inf))
    R = sp.diags(rng.uniform(0.5, 2.0, m))
    A2 = sp.csc_matrix(R @ A); A2.sort_indices()
    assert np.array_equal(A2.indptr, A.indptr) and np.array_equal(A2.indices, A.indices)
    ys2 = rng.standard_normal(m)
    zs2 = rng.uniform(0.0, 1.0, n) * (xs == 0.0)
    c2 = A2.T @ ys2 + zs2
    l2 = np.zeros(n); u2 = np.full(n, np.inf)
    u2[::5] = xs[::5] + 1.0
    free = np.arange(3, n, 11); l2[free] = -np.inf; c2[free] = (A2.T @ ys2)[free]
    lp2 = (A2, A2 @ xs, c2, l2, u2)
    return rb, lp1, lp2, float(c2 @ xs)


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["hsd", "mpc"])
@pytest.mark.parametrize("config", ["K1", "K2", "two_shards"])
def test_gpu_loops_reload_equals_a_fresh_load_bitwise(algo, config):
    from tulip_jl_amd.hsd_device import DeviceHSD
    from tulip_jl_amd.mpc_device import DeviceMPC
    cls = DeviceHSD if algo == "hsd" else DeviceMPC
    rb, lp1, lp2, zopt = block_angular_lp()
    kw = dict(device=0, row_block=rb, system="K2" if config == "K2" else "K1")
    if config == "two_shards":
        kw.update(ngpus=2, devices=[0, 0])
    L = _lib.lib()
    opt = cls(*lp1, **kw)
    opt.optimize()
    assert opt.status == "Trm_Optimal"
    tk.set_values(opt.kkt, lp2[0])                                             # bare: the loops' own copies of A and the LP data are stale
    assert L.tlpk_ipm_factor(opt.kkt._h, 1e-4, 1e-4) == _lib.BADARG and b"tlpk_ipm_reload" in L.tlpk_last_error(opt.kkt._h)
    assert L.tlpk_ipm_reset(opt.kkt._h) == _lib.BADARG
    x_old = np.empty(opt.n)
    assert L.tlpk_ipm_get(opt.kkt._h, 0, _lib.as_pd(x_old), opt.n) == _lib.OK   # the last iterate can still be read
    bytes1 = opt.kkt.stats()["device_bytes"]
    opt.reload(A=lp2[0], b=lp2[1], c=lp2[2], l=lp2[3], u=lp2[4])
    assert opt.kkt.stats()["device_bytes"] == bytes1
    opt.optimize()
    fresh = cls(*lp2, **kw)
    fresh.optimize()
    print(algo, config, opt.status, opt.niter, opt.primal_objective, "fresh:", fresh.status, fresh.niter, fresh.primal_objective)
    assert opt.status == fresh.status == "Trm_Optimal" and opt.niter == fresh.niter
    assert abs(fresh.primal_objective - zopt) <= 1e-6 * (1 + abs(zopt))
    assert same_bits(np.array([opt.primal_objective, opt.dual_objective]), np.array([fresh.primal_objective, fresh.dual_objective]))
    assert same_bits(opt._get(0, opt.n), fresh._get(0, fresh.n)) and same_bits(opt._get(5, opt.m), fresh._get(5, fresh.m))
    assert opt.p == fresh.p
    # all four NULL: same data, start over
    assert L.tlpk_ipm_reload(opt.kkt._h, None, None, None, None) == _lib.OK
    opt.optimize()
    assert opt.niter == fresh.niter and same_bits(opt._get(0, opt.n), fresh._get(0, fresh.n))
    # a handle that was never loaded
    bare = tk.setup(lp1[0], tk.K1(), tk.Backend(device=0, row_block=rb))
    assert L.tlpk_ipm_reload(bare._h, None, None, None, None) == _lib.BADARG and b"tlpk_ipm_load" in L.tlpk_last_error(bare._h)
    # tlpk_ipm_load twice keeps its refusal
    v = np.ones(opt.n)
    assert L.tlpk_ipm_load(opt.kkt._h, _lib.as_pd(np.ones(opt.m)), _lib.as_pd(v), _lib.as_pd(v), _lib.as_pd(v)) == _lib.BADARG


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["general", "block_angular"])
def test_gpu_refresh_after_graph_replay(kind, monkeypatch):
    """The captured graphs of the small-LP path name pair_w, Tx, Px ... by address: the refresh is in place, so a handle that has already
    replayed its graphs factorises and solves the new values through the same graphs."""
    monkeypatch.setenv("TLPK_GRAPH", "2" if kind == "block_angular" else "1")
    A, system, kw = CASES["k1_block" if kind == "block_angular" else "k1_general"]
    nz2 = second_values(A.nnz)
    m, n = A.shape
    th, rp, rd, xp, xd = ipm_like_data(m, n, 3)
    d = [DevBuf(v) for v in (th, rp, rd, xp, xd)]

    def step(k):
        o = [DevBuf(n, 0.0), DevBuf(m, 0.0)]
        for _ in range(2):                                                     # the second round replays the cached graphs
            k.update_device(d[0].ptr, d[1].ptr, d[2].ptr)
            k.solve_device(o[0].ptr, o[1].ptr, d[3].ptr, d[4].ptr)
        return [factor_entries(k, k.factor_panels()), o[0].get(), o[1].get()]

    kkt = tk.setup(A, system, tk.Backend(device=0, **kw))
    first = step(kkt)
    tk.set_values(kkt, nz2)
    second = step(kkt)
    want = step(tk.setup(with_values(A, nz2), system, tk.Backend(device=0, **kw)))
    assert all_same(second, want) and not all_same(second, first)
