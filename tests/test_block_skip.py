"""Block skip (`tlpk_block_skip`, `tk.block_skip`; DESIGN.md section 4b'-s): a direct handle whose matrix is block diagonal leaves a set of
blocks out of an update or a solve.  The skipped blocks' workgroups return at once, nothing they own is read or written, and the other
blocks get the bits of an unmasked call.

CPU (analyse-only handles): every refusal in its order with its sentence, a refused call leaves the mask alone, the `front_unit` table against
what the test derives from the symbolic arrays (K1 and K2), and the schedule arrays before and after a mask.

GPU: one block-diagonal stack of four blocks (row_block = block index) --
    0  workloads.general_sparse_lp(1400)          a multi-block-column top front: wide diagonal blocks, k_trsm, k_update, extend-add, the sweeps
    1  stair25 in standard form                   small fronts, thin solves, the small-front solve kernels
    2  general_sparse_lp(1400) again              a copy of block 0: tiles of both share the update launches
    3  helpers.random_lp_matrix(420, 700, 6, 11)  a small random block
The launch kinds the stack must contain are asserted (KINDS), so that a change of the analysis cannot quietly empty the test.  One of them is not
where the stack was expected to supply it: under K1 no front of the stack has 17 .. 64 pivot columns, so LK_POTRF (the one-block diagonal
kernel) is absent, and enlarging blocks 0 / 2 to general_sparse_lp(2600) does not change that (checked on an analyse-only handle); the same
stack under K2 has such fronts.  LK_POTRF is therefore asserted on the K2 handle, every other kind on both.  Under K1 the top fronts of
blocks 0 and 2 run in one dependency-driven launch (LK_CHAIN), so k_chain's skip is exercised by the stack as well as by the second shape
(two copies of test_chain.py's single-front LP under its environment).  The stack has no isolated 1 x 1 fronts; a small handle of its own
covers k_single_factor / k_single_solve.  All comparisons are bitwise."""
import functools
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import tulip_jl_amd as tk  # noqa: E402
from tulip_jl_amd import _lib  # noqa: E402
from helpers import DevBuf, block_angular, ipm_like_data, random_lp_matrix  # noqa: E402

LK = {"EXTEND_ADD": 0, "POTRF": 1, "TRSM": 2, "UPDATE": 3, "TRSM_THIN": 14, "FWD_SMALL": 15, "BWD_SMALL": 16, "POTRF_SMALL": 17, "FWD_SWEEP": 18,
      "BWD_SWEEP": 19, "CHAIN": 22}
KINDS = ["POTRF_SMALL", "POTRF", "TRSM", "TRSM_THIN", "UPDATE", "EXTEND_ADD", "FWD_SWEEP", "BWD_SWEEP", "FWD_SMALL", "BWD_SMALL"]


def _system(name):
    return tk.K2() if name == "K2" else tk.K1()


@functools.lru_cache(maxsize=None)
def stack():
    from workloads import general_sparse_lp
    from tulip_jl_amd.problem import read_free_mps, standard_form
    g = general_sparse_lp(1400)
    s25 = sp.csc_matrix(standard_form(read_free_mps(os.path.join(HERE, "golden", "stair25.mps"))).A)
    mats = [g, s25, g, random_lp_matrix(420, 700, 6, 11)]
    A = sp.block_diag(mats, format="csc")
    A.sort_indices()
    rb = np.repeat(np.arange(4), [M.shape[0] for M in mats]).astype(np.int64)
    return A, rb


@functools.lru_cache(maxsize=None)
def small_stack():
    A = sp.block_diag([random_lp_matrix(60, 120, 3, k) for k in range(4)], format="csc")
    A.sort_indices()
    return A, np.repeat(np.arange(4), 60).astype(np.int64)


def skip_call(kkt, mask, nblocks=None):
    """(return code, tlpk_last_error) of tlpk_block_skip; mask None = NULL."""
    L = _lib.lib()
    m8 = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    nb = nblocks if nblocks is not None else (len(m8) if m8 is not None else int(kkt.stats()["n_blocks"]))
    rc = L.tlpk_block_skip(kkt._h, None if m8 is None else _lib.as_pu8(m8), nb)
    return rc, L.tlpk_last_error(kkt._h).decode()


def col_units(A, rb):
    """Block of every column of a block-diagonal A (no empty columns)."""
    assert (np.diff(A.indptr) > 0).all()
    return rb[A.indices[A.indptr[:-1]]]


def expected_front_unit(kkt, A, rb, cu=None):
    """front_unit from perm, front_col0, front_ns, rowidx and the row -> block map: the unit of a front is the unit of its pivot columns; every row index of
    the front and its parent must agree (asserted here, as the library verifies it).  cu: the unit of every column where the rows cannot tell (a batch's
    column offsets: an LP may have empty columns), read for K2 only."""
    k2 = kkt.system == _lib.SYSTEM_K2
    n = A.shape[1]
    node_unit = np.concatenate([col_units(A, rb) if cu is None else cu, rb]) if k2 else rb                 # K2: node j < n is a column, node n + i a row
    perm = kkt.symbolic("perm")
    col0, ns, f, rowoff, parent = (kkt.symbolic(w) for w in ("front_col0", "front_ns", "front_f", "front_rowoff", "front_parent"))
    rowidx = kkt.symbolic("rowidx")
    assert len(perm) == (n + A.shape[0] if k2 else A.shape[0])
    fu = np.empty(len(col0), dtype=np.int64)
    for s in range(len(col0)):
        u = node_unit[perm[col0[s]:col0[s] + ns[s]]]
        rows = node_unit[perm[rowidx[rowoff[s]:rowoff[s] + f[s]]]]
        assert (u == u[0]).all() and (rows == u[0]).all(), s
        fu[s] = u[0]
    assert all(parent[s] < 0 or fu[parent[s]] == fu[s] for s in range(len(col0)))
    singles = kkt.symbolic("singles")
    nsg = (len(singles) - 2) // 3
    single_col = singles[2 * nsg:3 * nsg]
    return np.concatenate([fu, node_unit[perm[single_col]]]) if nsg else fu


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_listed():
    import re
    header = open(os.path.join(ROOT, "include", "tlpk.h")).read()
    for name in ("tlpk_block_skip", "tlpk_ipm_batch_skip"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name), name
    assert hasattr(tk, "block_skip")


def test_refusals_in_their_order_and_a_refused_call_leaves_the_mask():
    L = _lib.lib()
    A, rb = small_stack()
    B, rbl = block_angular(4, 60, 120, 90, 3, 0.5, 1)                     # with linking rows
    m4 = np.array([0, 1, 0, 1], dtype=np.uint8)
    # 1. h NULL
    assert L.tlpk_block_skip(None, _lib.as_pu8(m4), 4) == _lib.BADARG
    # 2. not a single-device direct handle -- each also wrong further down the list (refine_steps, linking rows, no row_block, nblocks): the kind is named first
    kinds = [("sharded", lambda: tk.setup(B, tk.K1(), tk.Backend(device=-1, row_block=rbl, rank=0, nranks=2))),
             ("dense-matrix", lambda: tk.setup(np.asfortranarray(A.toarray()), tk.K1(), tk.DenseBackend(device=-1))),
             ("Krylov", lambda: tk.setup(A, tk.K1(), tk.KrylovBackend(device=-1))),
             ("dense_cols", lambda: tk.setup(A, tk.K1(), tk.Backend(device=-1, row_block=rb, dense_cols=[3])))]
    for word, make in kinds:
        rc, msg = skip_call(make(), m4, 7)
        assert rc == _lib.BADARG and word in msg and "single-device direct" in msg, (word, msg)
    # 3. refine_steps > 0 (before: no row_block, wrong nblocks)
    rc, msg = skip_call(tk.setup(A, tk.K1(), tk.Backend(device=-1, refine=1)), m4, 7)
    assert rc == _lib.BADARG and "refine_steps" in msg
    # 5. no row_block / linking rows (before: wrong nblocks)
    rc, msg = skip_call(tk.setup(A, tk.K1(), tk.Backend(device=-1)), m4, 7)
    assert rc == _lib.BADARG and "no row_block" in msg
    for system in ("K1", "K2"):
        rc, msg = skip_call(tk.setup(B, _system(system), tk.Backend(device=-1, row_block=rbl)), m4, 7)
        assert rc == _lib.BADARG and "linking rows" in msg
    # 6. nblocks; 8. TLPK_NO_DEVICE after the structural checks, the table is built; the mask of an analyse-only handle stays empty throughout
    for system in ("K1", "K2"):
        kkt = tk.setup(A, _system(system), tk.Backend(device=-1, row_block=rb))
        assert (kkt.symbolic("front_unit") == -1).all() and len(kkt.symbolic("front_skip")) == 0 and kkt.symbolic("skip_bytes")[0] == 0
        for nb in (3, 5):
            rc, msg = skip_call(kkt, m4, nb)
            assert rc == _lib.BADARG and "n_blocks = 4" in msg
            assert (kkt.symbolic("front_unit") == -1).all()
        assert skip_call(kkt, m4)[0] == _lib.NO_DEVICE
        assert skip_call(kkt, None)[0] == _lib.NO_DEVICE
        assert (kkt.symbolic("front_unit") >= 0).all() and len(kkt.symbolic("front_skip")) == 0
        with pytest.raises(RuntimeError):
            tk.block_skip(kkt, m4)
    # 7. a front that is not contained in one block: K2, an empty column of A is a node of no block
    C0 = A.tolil(); C0[:, 5] = 0; C0 = sp.csc_matrix(C0); C0.eliminate_zeros(); C0.sort_indices()
    kkt = tk.setup(C0, tk.K2(), tk.Backend(device=-1, row_block=rb))
    rc, msg = skip_call(kkt, m4)
    assert rc == _lib.BADARG and "belongs to no block" in msg and (kkt.symbolic("front_unit") == -1).all()      # nothing is left half-built
    # tlpk_ipm_batch_skip: NULL, and a handle that is not batch-loaded
    assert L.tlpk_ipm_batch_skip(None, 1) == _lib.BADARG
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=-1, row_block=rb))
    assert L.tlpk_ipm_batch_skip(kkt._h, 1) == _lib.BADARG and b"not batch-loaded" in L.tlpk_last_error(kkt._h)
    assert L.tlpk_ipm_batch_skip(kkt._h, 0) == _lib.BADARG


@pytest.mark.parametrize("system", ["K1", "K2"])
def test_front_unit_equals_what_the_symbolic_arrays_say(system):
    for A, rb in (stack(), small_stack()):
        kkt = tk.setup(A, _system(system), tk.Backend(device=-1, row_block=rb))
        assert skip_call(kkt, np.zeros(4, dtype=np.uint8))[0] == _lib.NO_DEVICE
        got, want = kkt.symbolic("front_unit"), expected_front_unit(kkt, A, rb)
        assert np.array_equal(got, want)
        assert set(np.unique(got).tolist()) == {0, 1, 2, 3}


def test_the_stack_contains_the_launch_kinds_it_is_there_for():
    A, rb = stack()
    for system in ("K1", "K2"):
        kkt = tk.setup(A, _system(system), tk.Backend(device=-1, row_block=rb))
        have = set()
        for name in ("factor_launches", "fwd_launches", "bwd_launches"):
            have |= set(kkt.symbolic(name).reshape(-1, 3)[:, 0].tolist())
        missing = [k for k in KINDS if LK[k] not in have and not (k == "POTRF" and system == "K1")]      # (see the module's docstring)
        assert not missing, (system, missing)
        if system == "K1":
            assert LK["CHAIN"] in have and kkt.stats()["chain_launches"] > 0


@pytest.mark.parametrize("system", ["K1", "K2"])
def test_a_mask_changes_no_schedule_array(system):
    from test_schedule_identity import NAMES
    A, rb = stack()
    kkt = tk.setup(A, _system(system), tk.Backend(device=-1, row_block=rb))
    before = {name: kkt.symbolic(name).copy() for name in NAMES}
    assert skip_call(kkt, np.array([0, 1, 0, 1], dtype=np.uint8))[0] == _lib.NO_DEVICE
    assert (kkt.symbolic("front_unit") >= 0).all()
    for name in NAMES:
        assert np.array_equal(before[name], kkt.symbolic(name)), name


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------------
def pk_len(lda, ns):
    b = ns >> 6
    return ns * lda - 64 * b * (ns - 32 * b - 31) + 64 * b


class Rig:
    """A handle and its twin on one block-diagonal matrix, two sets of update data, device buffers, and the panel ranges of every unit."""

    def __init__(self, A, rb, system):
        self.A, self.rb, self.system = A, rb, system
        self.m, self.n = A.shape
        self.nb = int(rb.max()) + 1
        self.kkt = tk.setup(A, _system(system), tk.Backend(device=0, row_block=rb))
        self.twin = tk.setup(A, _system(system), tk.Backend(device=0, row_block=rb))
        self.cu = col_units(A, rb)
        self.data = [ipm_like_data(self.m, self.n, seed, regime="mid") for seed in (1, 2)]
        self.dev = [[DevBuf(v) for v in d] for d in self.data]              # theta, regP, regD, xi_p, xi_d
        self.F1 = self.F2 = None
        self._idx = None

    def unit_index(self, kkt=None):
        """Per unit: the positions of its fronts' panels in the factor storage."""
        if self._idx is None:
            kkt = kkt or self.kkt
            assert skip_call(kkt, np.zeros(self.nb, dtype=np.uint8))[0] == _lib.OK and skip_call(kkt, None)[0] == _lib.OK      # (builds front_unit)
            loff, lda, ns = (kkt.symbolic(w) for w in ("front_loff", "front_lda", "front_ns"))
            fu = kkt.symbolic("front_unit")[:len(loff)]
            assert np.array_equal(kkt.symbolic("front_unit"), expected_front_unit(kkt, self.A, self.rb))
            self._idx = [np.concatenate([np.arange(loff[s], loff[s] + pk_len(int(lda[s]), int(ns[s]))) for s in np.flatnonzero(fu == u)]) for u in range(self.nb)]
        return self._idx

    def update(self, kkt, which):
        th, rp, rd = self.dev[which][:3]
        kkt.update_device(th.ptr, rp.ptr, rd.ptr)

    def factors(self):
        """F1 = the handle's factor after an unmasked update with data set 0, F2 = the twin's after an unmasked update with data set 1."""
        if self.F1 is None:
            self.update(self.kkt, 0); self.F1 = self.kkt.factor_panels().copy()
            self.update(self.twin, 1); self.F2 = self.twin.factor_panels().copy()
        return self.F1, self.F2

    def same(self, F, G, units):
        idx = self.unit_index()
        return all(np.array_equal(F[idx[u]], G[idx[u]], equal_nan=True) for u in units)

    def solve(self, kkt, which):
        dx, dy = DevBuf(self.n), DevBuf(self.m)
        kkt.solve_device(dx.ptr, dy.ptr, self.dev[which][3].ptr, self.dev[which][4].ptr)
        return dx.get(), dy.get()

    def solve2(self, kkt):
        b = [DevBuf(self.n), DevBuf(self.m), DevBuf(self.n), DevBuf(self.m)]
        d0, d1 = self.dev
        kkt.solve2_device(b[0].ptr, b[1].ptr, d0[3].ptr, d0[4].ptr, b[2].ptr, b[3].ptr, d1[3].ptr, d1[4].ptr)
        return [v.get() for v in b]

    def seg_equal(self, got, ref, units):
        """(dx, dy) pairs: the segments of `units` are equal bit for bit"""
        units = sorted(units)
        cols, rows = np.isin(self.cu, units), np.isin(self.rb, units)
        assert cols.any() and rows.any()
        return np.array_equal(got[0][cols], ref[0][cols]) and np.array_equal(got[1][rows], ref[1][rows])

    def close(self):
        self.kkt.close(); self.twin.close()


_rigs = {}


def rig(system):
    if system not in _rigs:
        _rigs[system] = Rig(*stack(), system)
    return _rigs[system]


def check_update(r, skip):
    """Check 1: theta_1 unmasked, then theta_2 under the mask: the units that ran equal the twin's unmasked theta_2 factor, the skipped ones kept theta_1's."""
    F1, F2 = r.factors()
    run = [u for u in range(r.nb) if u not in skip]
    assert not r.same(F1, F2, range(r.nb)) and all(not r.same(F1, F2, [u]) for u in range(r.nb))       # (the two data sets differ on every unit)
    r.update(r.kkt, 0)
    tk.block_skip(r.kkt, [int(u in skip) for u in range(r.nb)])
    fs = r.kkt.symbolic("front_skip")
    assert np.array_equal(fs != 0, np.isin(r.kkt.symbolic("front_unit"), list(skip)))
    r.update(r.kkt, 1)
    F = r.kkt.factor_panels().copy()
    tk.block_skip(r.kkt, None)
    assert len(r.kkt.symbolic("front_skip")) == 0
    assert r.same(F, F2, run), "a unit that ran differs from the unmasked update"
    assert r.same(F, F1, skip), "a skipped unit's panels were touched"
    assert int(r.kkt.symbolic("chain_retries")[0]) == 0


def check_solve(r, skip):
    """Check 2: after an unmasked theta_2 update, masked solves give the units that ran the unmasked solve's bits; NULL restores everything."""
    run = [u for u in range(r.nb) if u not in skip]
    r.update(r.kkt, 1)
    ref0, ref1 = r.solve(r.kkt, 0), r.solve(r.kkt, 1)
    pair = r.solve2(r.kkt)
    assert r.seg_equal(pair[:2], ref0, range(r.nb)) and r.seg_equal(pair[2:], ref1, range(r.nb))
    tk.block_skip(r.kkt, [int(u in skip) for u in range(r.nb)])
    got0 = r.solve(r.kkt, 0)
    gp = r.solve2(r.kkt)
    tk.block_skip(r.kkt, None)
    for got, ref in ((got0, ref0), (gp[:2], ref0), (gp[2:], ref1)):
        assert r.seg_equal(got, ref, run)
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert not r.seg_equal(got0, ref0, skip)                                # (the skipped segments were indeed not solved)
    again = r.solve(r.kkt, 0)
    assert r.seg_equal(again, ref0, range(r.nb))
    assert r.seg_equal(r.solve2(r.kkt)[2:], ref1, range(r.nb))


@pytest.mark.gpu
@pytest.mark.parametrize("system", ["K1", "K2"])
def test_masked_update_and_solve_on_the_stack(system):
    r = rig(system)
    st = r.kkt.stats()
    print(system, "fronts", len(r.kkt.symbolic("front_ns")), "chain_launches", st["chain_launches"], "skip_bytes", int(r.kkt.symbolic("skip_bytes")[0]))
    before = st["device_bytes"]
    check_update(r, {1, 3})
    grown = r.kkt.stats()["device_bytes"] - before
    assert grown == int(r.kkt.symbolic("skip_bytes")[0]) > 0               # device_bytes grows once, by what the key reports
    check_solve(r, {1, 3})
    check_update(r, {0, 2})                                                 # the other half: the big fronts (and the chain's items) are the skipped ones
    check_solve(r, {0})
    assert r.kkt.stats()["device_bytes"] - before == grown


@pytest.mark.gpu
def test_a_bad_unit_cannot_fail_the_others():
    r = rig("K1")
    _, F2 = r.factors()
    th, rp, rd = (v.copy() for v in r.data[1][:3])
    th[r.cu == 3] = -1.0                                                    # theta^-1 + regP < 0 on the columns of unit 3 only
    dth = DevBuf(th)
    tk.block_skip(r.kkt, None)
    with pytest.raises(tk.PosDefException):
        r.kkt.update_device(dth.ptr, r.dev[1][1].ptr, r.dev[1][2].ptr)
    fail = r.kkt.stats()["fail_col"]
    assert r.rb[r.kkt.perm()[fail]] == 3
    tk.block_skip(r.kkt, [0, 0, 0, 1])
    r.kkt.update_device(dth.ptr, r.dev[1][1].ptr, r.dev[1][2].ptr)           # TLPK_OK: the failing pivots belong to fronts that did not run
    F = r.kkt.factor_panels().copy()
    tk.block_skip(r.kkt, None)
    assert r.kkt.stats()["fail_col"] < 0
    assert r.same(F, F2, [0, 1, 2])


@pytest.mark.gpu
def test_everything_skipped_changes_nothing():
    r = rig("K1")
    F1, _ = r.factors()
    r.update(r.kkt, 0)
    tk.block_skip(r.kkt, [1, 1, 1, 1])
    r.update(r.kkt, 1)
    F = r.kkt.factor_panels().copy()
    dx, dy = r.solve(r.kkt, 0)
    pair = r.solve2(r.kkt)
    tk.block_skip(r.kkt, None)
    assert np.array_equal(F, F1, equal_nan=True)
    assert np.array_equal(r.kkt.factor_panels(), F1, equal_nan=True)
    assert all(np.isfinite(v).all() for v in (dx, dy, *pair))


@pytest.mark.gpu
def test_chain_shape_one_of_two_fronts_skipped(monkeypatch):
    from test_chain import _single_front_lp
    monkeypatch.setenv("TLPK_MACRO_TILES", "50")
    monkeypatch.setenv("TLPK_CHAIN_MIN_NS", "257")
    g = _single_front_lp(1500)
    A = sp.block_diag([g, g], format="csc"); A.sort_indices()
    r = Rig(A, np.repeat(np.arange(2), g.shape[0]).astype(np.int64), "K1")
    st = r.kkt.stats()
    assert st["chain_launches"] > 0 and st["chain_items"] > 0
    check_update(r, {1})
    check_update(r, {0})
    check_solve(r, {1})
    assert int(r.kkt.symbolic("chain_retries")[0]) == 0
    r.close()


@pytest.mark.gpu
def test_isolated_fronts_are_skipped_with_their_block(system="K1"):
    """Blocks with isolated 1 x 1 fronts (rows that share no column with another row): k_single_factor / k_single_solve and their bytes of front_skip.
    K1 only: under K2 such a row is a two-node front (the row and its column)."""
    A = sp.block_diag([sp.block_diag([random_lp_matrix(40, 70, 3, k), sp.identity(3)]) for k in range(3)], format="csc")
    A.sort_indices()
    r = Rig(A, np.repeat(np.arange(3), 43).astype(np.int64), system)
    nsg = (len(r.kkt.symbolic("singles")) - 2) // 3
    assert nsg >= 9
    check_update(r, {1})
    check_solve(r, {0, 2})
    r.close()


@pytest.mark.gpu
def test_refusals_that_need_a_device():
    from test_hsd_batch import load_batch, stacked_handle
    A, ro, co, vecs = stacked_handle()
    rb = np.repeat(np.arange(3), np.diff(ro)).astype(np.int64)
    L = _lib.lib()
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=0, row_block=rb))
    assert load_batch(kkt, 3, ro, co, vecs)[0] == _lib.OK
    rc, msg = skip_call(kkt, np.zeros(3, dtype=np.uint8), 7)               # 4. batch-loaded (before: wrong nblocks)
    assert rc == _lib.BADARG and "batch owns the mask" in msg
    assert L.tlpk_ipm_batch_skip(kkt._h, 1) == _lib.OK and L.tlpk_ipm_batch_skip(kkt._h, 0) == _lib.OK
    assert np.array_equal(kkt.symbolic("front_unit"), expected_front_unit(kkt, A, rb)) and len(kkt.symbolic("front_skip")) == 0
    kkt.close()
    # a mask and a table from before the load: blocks that are not the LPs (LP 1 and LP 2 form block 1).  The load lifts the mask, the batch rebuilds the table
    rb2 = np.minimum(rb, 1)
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=0, row_block=rb2))
    tk.block_skip(kkt, [1, 0])
    assert np.array_equal(kkt.symbolic("front_unit"), expected_front_unit(kkt, A, rb2)) and kkt.symbolic("front_skip").any()
    assert load_batch(kkt, 3, ro, co, vecs)[0] == _lib.OK and len(kkt.symbolic("front_skip")) == 0
    assert L.tlpk_ipm_batch_skip(kkt._h, 1) == _lib.OK
    assert np.array_equal(kkt.symbolic("front_unit"), expected_front_unit(kkt, A, rb))
    kkt.close()
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=0, row_block=rb, refine=1))
    assert load_batch(kkt, 3, ro, co, vecs)[0] == _lib.OK
    assert L.tlpk_ipm_batch_skip(kkt._h, 1) == _lib.BADARG and b"refine_steps" in L.tlpk_last_error(kkt._h)
    rc, msg = skip_call(kkt, np.zeros(3, dtype=np.uint8))
    assert rc == _lib.BADARG and "refine_steps" in msg                     # 3. before 4.
    kkt.close()
