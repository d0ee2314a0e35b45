"""A batch that keeps going (`tlpk_ipm_batch_refill`, `tlpk_ipm_get_lp`, `BatchedDeviceHSD.refill` / `optimize_stream`,
`Model.optimize_batch(slots=...)`): when an LP of a batch-loaded handle is decided the next LP of a queue takes its slot while every other
slot continues.  CPU: the ABI surface, the refusals in their order, the pattern key and the FIFO slot assignment as pure functions, the
refusals of the Python layer.  GPU: a refilled slot equals a fresh load bit for bit (K1, K2; values and vectors, vectors only, values
only); unselected LPs keep every bit; an LP that streams through a slot is the LP of a plain batch in that slot, bit for bit; the pass
count beats successive batches; two patterns in one handle; options travel with the LP; the Model front door."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import tulip_jl_amd as tk
from ipm_harness import read_free_mps, standard_form
from test_hsd_batch import EXAMPLE_STATUS, EXAMPLES, GOLDEN, ROOT, golden, load_batch, small_lps, stacked_handle
from tulip_jl_amd import _lib
from tulip_jl_amd.hsd_batch import BatchedDeviceHSD, pattern_key, stream_assign
from tulip_jl_amd.hsd_device import Options

STREAM_SYMBOLS = ["tlpk_ipm_batch_refill", "tlpk_ipm_get_lp"]


def family(N, m=12, n=30, seed=5):
    """N LPs on one 12 x 30 pattern with differing iteration counts and all three outcomes (optimal, primal infeasible, dual infeasible)."""
    rng = np.random.default_rng(seed)
    pat = sp.random(m, n, density=0.3, random_state=np.random.RandomState(seed), format="csc"); pat.data[:] = 1.0
    pat = (pat + sp.csc_matrix((np.ones(m), (np.arange(m), np.arange(m))), shape=(m, n))).tocsc(); pat.sort_indices()
    out = []
    for j in range(N):
        A = pat.copy(); A.data = rng.standard_normal(A.nnz) * 10.0 ** rng.uniform(-j / 3, j / 3, A.nnz)
        l = np.zeros(n); u = np.full(n, np.inf); u[::3] = 5.0; l[1] = -np.inf
        b = A @ rng.uniform(0.5, 2.0, n)
        c = A.T @ rng.standard_normal(m) + rng.uniform(0.1, 1.0, n) * (1 if j % 4 != 3 else -1)
        if j % 5 == 4: b = b + 100.0 * np.abs(b).max() * (np.arange(m) == 0)
        out.append((A, b, c, l, u))
    return out


def bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def refill_call(kkt, slots, nz, vecs):
    ptr = lambda a: None if a is None else _lib.as_pd(a)         # noqa: E731
    rc = _lib.lib().tlpk_ipm_batch_refill(kkt._h, None if slots is None else _lib.as_pu8(slots), ptr(nz), 0 if nz is None else nz.shape[0],
                                          *[ptr(v) for v in vecs])
    return rc, _lib.lib().tlpk_last_error(kkt._h).decode()


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_stream_symbols_are_declared_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "tlpk.h")).read()
    L = _lib.lib()
    for name in STREAM_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name


def test_refill_and_get_lp_refuse_in_order_without_a_load():
    A, ro, co, vecs = stacked_handle()
    L = _lib.lib()
    sel = np.array([0, 1, 0], dtype=np.uint8)
    nz = A.data.copy()
    x = np.zeros(9)
    assert L.tlpk_ipm_batch_refill(None, _lib.as_pu8(sel), None, 0, None, None, None, None) == _lib.BADARG
    assert L.tlpk_ipm_get_lp(None, 0, 1, _lib.as_pd(x), 9) == _lib.BADARG
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=-1, row_block=np.repeat(np.arange(3), np.diff(ro))))      # analyse-only, nothing loaded
    for slots, values in ((sel, nz), (None, nz), (None, nz[:-1]), (sel, nz[:-1])):      # "load first" comes before the NULL slots and the length of nzval
        rc, msg = refill_call(kkt, slots, values, vecs)
        assert rc == _lib.BADARG and "load first" in msg, msg
    assert load_batch(kkt, 3, ro, co, vecs)[0] == _lib.NO_DEVICE                      # (an analyse-only handle is never loaded)
    rc, msg = refill_call(kkt, sel, nz, vecs)
    assert rc == _lib.BADARG and "load first" in msg
    assert L.tlpk_ipm_get_lp(kkt._h, 0, 1, _lib.as_pd(x), 9) in (_lib.BADARG, _lib.NO_DEVICE)      # as tlpk_ipm_get on this handle
    assert L.tlpk_ipm_get_lp(kkt._h, 0, 1, _lib.as_pd(x), 9) == L.tlpk_ipm_get(kkt._h, 0, _lib.as_pd(np.zeros(20)), 20)
    kkt.close()


def test_pattern_key_and_slot_assignment_are_pure_functions():
    fam = family(2)
    A0, A1 = fam[0][0], fam[1][0]
    assert pattern_key(A0) == pattern_key(A1)                          # values do not count
    assert pattern_key(A0) == pattern_key(A0.toarray() != 0) == pattern_key(sp.coo_matrix(A0))
    moved = A0.tolil(); i, j = [(i, j) for i in range(12) for j in range(30) if A0[i, j] == 0][0]
    i2 = A0[:, j].nonzero()[0][0]
    moved[i, j] = moved[i2, j]; moved[i2, j] = 0
    moved = moved.tocsc(); moved.eliminate_zeros()
    assert moved.nnz == A0.nnz and pattern_key(moved) != pattern_key(A0)
    wide = sp.hstack([A0, sp.csc_matrix((12, 1))]).tocsc()
    assert wide.nnz == A0.nnz and pattern_key(wide) != pattern_key(A0)
    assert pattern_key(A0.T.tocsc()) != pattern_key(A0)
    # the stacked handle's slots carry the keys of the LPs they were analysed with
    lps = [fam[0], small_lps()[0], fam[1]]
    opt = BatchedDeviceHSD(lps, device=-1, load=False)
    assert [opt.slot_key(k) for k in range(3)] == [pattern_key(lp[0]) for lp in lps]
    opt.kkt.close()
    # FIFO: every free slot, in slot order, takes the first waiting LP of its own pattern
    P, Q = "P", "Q"
    slot_keys = [P, P, Q]
    assert stream_assign({0, 1, 2}, slot_keys, [Q, P, Q, P, P]) == [(0, 1), (1, 3), (2, 0)]
    assert stream_assign({2, 0}, slot_keys, [P, P, P]) == [(0, 0)]            # no Q left: slot 2 stays parked
    assert stream_assign({1}, slot_keys, [Q, Q, P]) == [(1, 2)]
    assert stream_assign({2}, slot_keys, [P, Q, Q]) == [(2, 1)]
    assert stream_assign(set(), slot_keys, [P, Q]) == [] and stream_assign({0, 1, 2}, slot_keys, []) == []


def test_python_refusals_need_no_gpu():
    fam = family(4)
    opt = BatchedDeviceHSD(fam[:2], device=-1, load=False)
    with pytest.raises(RuntimeError, match="nothing is loaded"):
        opt.optimize()
    with pytest.raises(RuntimeError, match="nothing is loaded"):
        opt.optimize_stream(fam[2:])
    with pytest.raises(RuntimeError, match="nothing is loaded"):
        opt.refill([1], [fam[2]])
    other = small_lps()[0]
    before = (opt.A.data.copy(), opt._b.copy(), opt._c.copy(), opt._l.copy(), opt._u.copy())
    with pytest.raises(ValueError, match="pattern"):
        opt.refill([0, 1], [fam[3], other])
    with pytest.raises(ValueError, match="pattern"):
        opt.optimize_stream([fam[2], other, fam[3]])
    for a, b in zip(before, (opt.A.data, opt._b, opt._c, opt._l, opt._u)):
        assert bits(a, b)                                                # nothing was changed
    opt.kkt.close()
    paths = [os.path.join(GOLDEN, name + ".mps") for name in EXAMPLES[:2]]
    with pytest.raises(ValueError, match="mpc"):
        tk.Model.optimize_batch([tk.Model.load(p, algorithm="mpc") for p in paths], slots=2, device=-1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------------
def boundary_slots(seed, shapes=((1, 1), (9, 257), (8, 256))):
    """Three LPs at the segment boundaries of the block tables: 1 x 1, 9 x 257 (two blocks of a column kernel, a row group with one live row), 8 x 256."""
    rng = np.random.default_rng(seed)
    out = []
    for (m, n) in shapes:
        pat = sp.random(m, n, density=min(1.0, 6.0 / m), random_state=np.random.RandomState(7), format="csc"); pat.data[:] = 1.0
        pat = (pat + sp.csc_matrix((np.ones(m), (np.arange(m), np.arange(m))), shape=(m, n))).tocsc(); pat.sort_indices()
        A = pat.copy(); A.data = rng.uniform(0.5, 2.0, A.nnz) * rng.choice([-1.0, 1.0], A.nnz)
        l = np.zeros(n); u = np.full(n, np.inf); u[::3] = 4.0
        if n > 1: l[1] = -np.inf
        out.append((A, A @ rng.uniform(0.5, 2.0, n), rng.standard_normal(n), l, u))
    return out


def get_all(kkt, codes):
    L = _lib.lib()
    out = {}
    for what in codes:
        v = np.empty(kkt.m if what in _lib.IPM_GET_ROWS else kkt.n)
        assert L.tlpk_ipm_get(kkt._h, what, _lib.as_pd(v), v.shape[0]) == _lib.OK, what
        out[what] = v
    return out


def residuals_and_factor(kkt, nlp):
    L = _lib.lib()
    res = np.zeros(13 * nlp); fail = C.c_int64(7)
    one = np.ones(nlp); act = np.ones(nlp, dtype=np.uint8)
    assert L.tlpk_ipm_batch_residuals(kkt._h, _lib.as_pd(one), _lib.as_pd(res)) == _lib.OK
    assert L.tlpk_ipm_batch_factor(kkt._h, _lib.as_pu8(act), _lib.as_pd(one), _lib.as_pd(one), C.byref(fail)) == _lib.OK
    return res


def same_as_fresh(kkt, lps, system, label):
    """Everything the issue lists, bit for bit, against a handle created and batch-loaded on `lps`."""
    from test_set_values import factor_entries
    A, ro, co, vecs = stacked_handle(lps)
    fresh = tk.setup(A, system, tk.Backend(device=0, row_block=np.repeat(np.arange(len(lps)), np.diff(ro))))
    assert load_batch(fresh, len(lps), ro, co, vecs)[0] == _lib.OK
    a, b = get_all(kkt, range(6)), get_all(fresh, range(6))
    for what in range(6):
        assert bits(a[what], b[what]), (label, "start", what)
    ra, rb = residuals_and_factor(kkt, len(lps)), residuals_and_factor(fresh, len(lps))
    assert bits(ra, rb), (label, "residuals", ra - rb)
    codes = [18, 19, 20, 21, 33, 34, 35]
    a, b = get_all(kkt, codes), get_all(fresh, codes)
    for what in codes:
        assert bits(a[what], b[what]), (label, what)
    fa, fb = factor_entries(kkt, kkt.factor_panels()), factor_entries(fresh, fresh.factor_panels())
    assert fa.size > 0 and bits(fa, fb), (label, "factor", np.abs(fa - fb).max())
    fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sysname", ["K1", "K2"])
def test_a_refilled_slot_equals_a_fresh_load(sysname):
    system = tk.K1() if sysname == "K1" else tk.K2()
    L = _lib.lib()
    lps = boundary_slots(1)
    new1, new2 = boundary_slots(2)[1], boundary_slots(3)[1]
    A, ro, co, vecs = stacked_handle(lps)
    kkt = tk.setup(A, system, tk.Backend(device=0, row_block=np.repeat(np.arange(3), np.diff(ro))))
    sel = np.array([0, 1, 0], dtype=np.uint8)
    nz = A.data.copy()
    # refusals that need a device: not loaded, then (loaded) NULL slots, the length of nzval, no slot selected
    rc, msg = refill_call(kkt, sel, nz, vecs); assert rc == _lib.BADARG and "load first" in msg
    assert load_batch(kkt, 3, ro, co, vecs)[0] == _lib.OK
    rc, msg = refill_call(kkt, None, nz[:-1], vecs); assert rc == _lib.BADARG and "slots" in msg
    rc, msg = refill_call(kkt, sel, nz[:-1], vecs); assert rc == _lib.BADARG and "len" in msg
    start = get_all(kkt, range(6))
    assert refill_call(kkt, np.zeros(3, dtype=np.uint8), nz, [v + 1.0 for v in vecs])[0] == _lib.OK
    now = get_all(kkt, range(6))
    assert all(bits(start[w], now[w]) for w in range(6))
    x = np.zeros(257)
    assert L.tlpk_ipm_get_lp(kkt._h, 0, 3, _lib.as_pd(x), 257) == _lib.BADARG and L.tlpk_ipm_get_lp(kkt._h, 0, -1, _lib.as_pd(x), 257) == _lib.BADARG
    assert L.tlpk_ipm_get_lp(kkt._h, 0, 1, _lib.as_pd(x), 256) == _lib.BADARG and L.tlpk_ipm_get_lp(kkt._h, 5, 1, _lib.as_pd(x), 257) == _lib.BADARG
    assert L.tlpk_ipm_get_lp(kkt._h, 36, 1, _lib.as_pd(x), 257) == _lib.BADARG
    assert L.tlpk_ipm_get_lp(kkt._h, 1, 1, _lib.as_pd(x), 257) == _lib.OK and bits(x, start[1][1:258])
    same_as_fresh(kkt, lps, system, "as loaded")                       # (also: the handle has iterated once before the first refill)

    def stacked(mid_A, mid_vecs):
        cur = [lps[0], (mid_A,) + tuple(mid_vecs), lps[2]]
        return cur, stacked_handle(cur)

    # 1. values and vectors: one bound moves from finite to infinite, one the other way
    A1, (b1, c1, l1, u1) = new1[0], [v.copy() for v in new1[1:]]
    assert np.isfinite(u1[0]) and np.isinf(u1[2]) and np.isinf(l1[1]) and np.isfinite(l1[4])
    u1[0] = np.inf; u1[2] = 3.0; l1[1] = -1.0; l1[4] = -np.inf
    cur, (As, _, _, vs) = stacked(A1, (b1, c1, l1, u1))
    # only the selected LP's segments may be read: everything else of the arrays is poisoned
    poison_nz = np.full(As.nnz, np.nan); p0, p1 = As.indptr[co[1]], As.indptr[co[2]]; poison_nz[p0:p1] = As.data[p0:p1]
    poison = []
    for v, off in zip(vs, (ro, co, co, co)):
        w = np.full(v.shape, np.nan); w[off[1]:off[2]] = v[off[1]:off[2]]; poison.append(w)
    assert refill_call(kkt, sel, poison_nz, poison)[0] == _lib.OK
    same_as_fresh(kkt, cur, system, "values and vectors")
    # 2. vectors only
    b2, c2, l2, u2 = [v.copy() for v in new2[1:]]
    cur, (As, _, _, vs) = stacked(A1, (b2, c2, l2, u2))
    assert refill_call(kkt, sel, None, vs)[0] == _lib.OK
    same_as_fresh(kkt, cur, system, "vectors only")
    # 3. values only
    cur, (As, _, _, vs) = stacked(new2[0], (b2, c2, l2, u2))
    assert refill_call(kkt, sel, As.data.copy(), [None] * 4)[0] == _lib.OK
    same_as_fresh(kkt, cur, system, "values only")
    # a whole-handle tlpk_set_values makes the handle stale for the refill as for the other batch calls
    assert L.tlpk_set_values(kkt._h, _lib.as_pd(nz), nz.shape[0]) == _lib.OK
    rc, msg = refill_call(kkt, sel, None, vs); assert rc == _lib.BADARG and "tlpk_ipm_reload" in msg
    kkt.close()


@pytest.mark.gpu
def test_unselected_lps_are_not_touched():
    fam = family(4)
    opt = BatchedDeviceHSD(fam[:3], device=0)
    opt._call(opt.L.tlpk_ipm_reset(opt.kkt._h)); opt._init_state()
    act = opt.active; act[:] = True
    with np.errstate(all="ignore"):
        for _ in range(2):
            opt.compute_residuals(act); opt.update_solver_status(act)
            assert opt.compute_step(act).all()
            opt.niter[act] += 1
    read = lambda: {(k, what): opt._get_lp(k, what) for k in (0, 2) for what in range(33)}      # noqa: E731
    before, mid = read(), opt._get_lp(1, 0)
    host = {name: getattr(opt, name).copy() for name in ("tau", "kappa", "mu", "regP", "niter")}
    opt.refill([1], [fam[3]])
    after = read()
    for key in before:
        assert np.array_equal(before[key], after[key]) and bits(before[key], after[key]), key
    assert mid.any() and not opt._get_lp(1, 0).any()                      # slot 1 is back at the starting point
    for name, v in host.items():
        assert np.array_equal(np.delete(v, 1), np.delete(getattr(opt, name), 1)), name
    assert opt.tau[1] == opt.regP[1] == 1.0 and opt.niter[1] == 0 and opt.status[1] == "Trm_Unknown"
    opt.kkt.close()


_cache = {}
COMPARED = ("x", "y", "zl", "zu")


def plain_records(first, queue, records, system, options=None):
    """Every LP of first + queue in a plain BatchedDeviceHSD(...).optimize() of len(first) LPs, in the slot it streamed through (the other slots of
    a run hold LPs that streamed through THEM, or the slot's first occupant): what the stream is held to."""
    lps = list(first) + list(queue)
    opts = options or [Options()] * len(lps)
    todo, out = list(range(len(lps))), [None] * len(lps)
    while todo:
        run = {}
        for i in todo:
            run.setdefault(records[i]["slot"], i)
        todo = [i for i in todo if i not in run.values()]
        members = [run.get(k, k) for k in range(len(first))]
        opt = BatchedDeviceHSD([lps[i] for i in members], system=system, device=0, options=[opts[i] for i in members]).optimize()
        for k, i in run.items():
            sol = opt.solution(k)
            out[i] = dict(sol, zl=opt._get(k, 3), zu=opt._get(k, 4), tau=float(opt.tau[k]), timers=opt.timers_of(k), regP=float(opt.regP[k]))
        opt.kkt.close()
    return out


def assert_same_run(rec, ref, label):
    print(f"  {label}: slot {rec['slot']} passes {rec['entered']}..{rec['left']}  {rec['status']:22s} niter {rec['niter']:3d} / {ref['niter']:3d}  "
          f"n_bump {rec['timers']['n_bump']} / {ref['timers']['n_bump']}  z {rec['z_primal']:.12e} / {ref['z_primal']:.12e}")
    assert rec["status"] == ref["status"] and rec["niter"] == ref["niter"], label
    assert rec["timers"]["n_bump"] == ref["timers"]["n_bump"], label
    assert rec["primal_status"] == ref["primal_status"] and rec["dual_status"] == ref["dual_status"], label
    for key in COMPARED:
        assert bits(rec[key], ref[key]), (label, key, np.abs(rec[key] - ref[key]).max())
    assert bits(rec["tau"], ref["tau"]) and bits(rec["z_primal"], ref["z_primal"]) and bits(rec["z_dual"], ref["z_dual"]), label


def family_stream(system):
    if system not in _cache:
        fam = family(10)
        opt = BatchedDeviceHSD(fam[:3], system=system, device=0)
        records = opt.optimize_stream(fam[3:])
        _cache[system] = (fam, records, opt.passes)
        opt.kkt.close()
    return _cache[system]


@pytest.mark.gpu
@pytest.mark.parametrize("system", ["K1", "K2"])
def test_streaming_equals_solving(system):
    fam, records, passes = family_stream(system)
    assert len(records) == 10 and [r["slot"] for r in records[:3]] == [0, 1, 2] and all(r["entered"] == 1 for r in records[:3])
    ref = plain_records(fam[:3], fam[3:], records, system)
    print(system, "passes", passes)
    for i, (rec, r) in enumerate(zip(records, ref)):
        assert_same_run(rec, r, f"LP {i}")
    status = [r["status"] for r in records]
    assert "Trm_PrimalInfeasible" in status and "Trm_DualInfeasible" in status and "Trm_Optimal" in status, status      # guards the inputs
    assert len({r["niter"] for r in records}) > 2, "bad test input: the LPs should differ in length"


@pytest.mark.gpu
def test_streaming_needs_fewer_passes_than_successive_batches():
    fam, records, passes = family_stream("K1")
    dur = [r["niter"] + 1 for r in records]
    free_at = [0, 0, 0]                                                   # FIFO list scheduling on 3 slots: the next LP takes the slot that is free first
    for d in dur:
        k = free_at.index(min(free_at))
        free_at[k] += d
    makespan = max(free_at)
    batches = sum(max(dur[i:i + 3]) for i in range(0, 10, 3))             # the four successive batches (3, 3, 3, 1)
    print("niter", [d - 1 for d in dur], "passes", passes, "list-scheduling makespan", makespan, "successive batches", batches)
    assert passes <= makespan
    assert passes < batches
    for r in records:                                                     # the recorded passes are the schedule
        assert r["left"] - r["entered"] + 1 == r["niter"] + 1


@pytest.mark.gpu
def test_two_patterns_in_one_handle():
    fam = family(7)
    rng = np.random.default_rng(17)
    q0 = small_lps()[0]

    def q_lp(scale):
        A = q0[0].copy(); A.data = A.data * (1.0 + scale * rng.uniform(-1.0, 1.0, A.nnz))
        return (A,) + tuple(q0[1:])

    qs = [q0, q_lp(0.1), q_lp(0.2)]
    first = [fam[0], fam[1], qs[0]]
    queue = [fam[2], qs[1], fam[3], qs[2], fam[4], fam[5], fam[6]]      # interleaved
    opt = BatchedDeviceHSD(first, device=0)
    records = opt.optimize_stream(queue)
    is_q = [False, False, True, False, True, False, True, False, False, False]
    for rec, q in zip(records, is_q):
        assert (rec["slot"] == 2) == q, (rec["slot"], q)                  # every LP ran in a slot of its own pattern
    ref = plain_records(first, queue, records, "K1")
    for i, (rec, r) in enumerate(zip(records, ref)):
        assert_same_run(rec, r, f"LP {i}{' (Q)' if is_q[i] else ''}")
    last_q = max(rec["left"] for rec, q in zip(records, is_q) if q)
    print("passes", opt.passes, "last Q leaves in pass", last_q)
    assert opt.passes > last_q                                            # Q's slot stays parked while P's go on
    assert all(rec["left"] <= opt.passes for rec in records) and max(rec["left"] for rec in records) == opt.passes
    opt.kkt.close()


@pytest.mark.gpu
def test_a_failed_lp_frees_its_slot_and_options_travel_with_the_lp():
    from test_ipm_harness import random_feasible_lp

    class TwoIterations(Options):
        IterationsLimit = 2

    d = standard_form(random_feasible_lp(81, 200, 23))
    rng = np.random.default_rng(4)
    succ = (d.A, d.b, d.c * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, d.c.shape[0])), d.l, d.u, d.c0, d.objsense)
    first = [d, golden("lpex_opt")]
    opts = [TwoIterations(), Options()]
    opt = BatchedDeviceHSD(first, options=opts, device=0)
    records = opt.optimize_stream([succ])
    assert records[0]["status"] == "Trm_IterationLimit" and records[0]["niter"] == 2 and records[0]["left"] == 3
    assert records[2]["slot"] == 0 and records[2]["entered"] == 4
    assert records[2]["status"] == "Trm_Optimal" and records[2]["niter"] > 2
    assert records[1]["status"] == "Trm_Optimal"
    ref = plain_records(first, [succ], records, "K1", options=opts + [Options()])
    for i, (rec, r) in enumerate(zip(records, ref)):
        assert_same_run(rec, r, f"LP {i}")
    assert opt.regP[0] == ref[2]["regP"]                                   # the regularisations restarted at 1 with the new LP
    assert opt.opts[0].IterationsLimit == Options().IterationsLimit and opt._o["IterationsLimit"][0] == Options().IterationsLimit
    opt.kkt.close()


@pytest.mark.gpu
def test_model_optimize_batch_with_slots():
    paths = [os.path.join(GOLDEN, name + ".mps") for name in EXAMPLES] + [os.path.join(GOLDEN, "lpex_opt.mps")] * 2

    def load(**kw):
        models = [tk.Model.load(p, **kw) for p in paths]
        for mdl, f in zip(models[4:], (1.03, 0.96)):
            mdl.lp.obj = mdl.lp.obj * f
        return models

    own = [m.optimize() for m in load(device=0)]
    models = tk.Model.optimize_batch(load(), slots=2, device=0)
    print([(m.status, m.inner is None) for m in own])
    for a, b in zip(models, own):
        assert a.status == b.status
        assert (a.inner is None) == (b.inner is None)            # (a model presolve alone solves never reaches the batch)
        for f in ("objective_value", "dual_objective_value"):
            za, zb = getattr(a, f)(), getattr(b, f)()
            assert (za == zb) or abs(za - zb) <= 1e-9 * (1 + abs(zb)), (f, za, zb)
    assert [m.status for m in own[:4]] == EXAMPLE_STATUS and [m.status for m in own[4:]] == ["Trm_Optimal"] * 2
    assert sum(m.inner is not None for m in models) >= 3, "bad test input: the stream needs more LPs than slots"
