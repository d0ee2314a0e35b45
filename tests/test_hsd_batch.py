"""Batched device-resident HSD (`tlpk_ipm_load_batch`, `tlpk_ipm_batch_*`, `BatchedDeviceHSD`, `Model.optimize_batch`): B LPs stacked into one
block-diagonal handle, the interior-point loop with per-LP scalars and masks.  CPU: the ABI surface, the argument checks of the load in their
order, the refusals, the stacking.  GPU: a one-LP batch is the unbatched loop bit for bit; in a mixed batch every LP converges and reports as
its own `DeviceHSD` run does; segment boundaries (1 x 1, 256 / 257 columns, 8 k + 1 rows); determinism and independence of the batch's
composition; the per-LP retry loop; parking of finished and failed LPs; reload; the Model front door."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import tulip_jl_amd as tk
from ipm_harness import LP, read_free_mps, standard_form
from tulip_jl_amd import _lib
from tulip_jl_amd.hsd_batch import BatchedDeviceHSD
from tulip_jl_amd.hsd_device import DeviceHSD, Options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SQRT_EPS = float(np.sqrt(np.finfo(float).eps))
BATCH_SYMBOLS = ["tlpk_ipm_load_batch", "tlpk_ipm_batch_residuals", "tlpk_ipm_batch_factor", "tlpk_ipm_batch_hsolve_newton",
                 "tlpk_ipm_batch_newton", "tlpk_ipm_batch_targets", "tlpk_ipm_batch_accept", "tlpk_ipm_batch_advance"]
EXAMPLES = ["lpex_opt", "lpex_inf", "lpex_ubd", "lpex_freevars"]
EXAMPLE_STATUS = ["Trm_Optimal", "Trm_PrimalInfeasible", "Trm_DualInfeasible", "Trm_Optimal"]


def golden(name):
    return standard_form(read_free_mps(os.path.join(GOLDEN, name + ".mps")))


def small_lps():
    """Three standard-form LPs of different sizes (3 x 7, 5 x 9, 2 x 4) with finite, infinite and mixed bounds."""
    rng = np.random.default_rng(11)
    out = []
    for (m, n) in ((3, 7), (5, 9), (2, 4)):
        A = sp.csc_matrix(rng.standard_normal((m, n)))
        l = np.zeros(n); u = np.full(n, np.inf)
        u[::3] = 2.0 + m
        l[1] = -np.inf
        out.append((A, rng.standard_normal(m) * (m + 1), rng.standard_normal(n) * n, l, u))
    return out


def stacked_handle(lps=None, **kw):
    lps = lps or small_lps()
    A = sp.block_diag([p[0] for p in lps], format="csc")
    ro = np.concatenate([[0], np.cumsum([p[0].shape[0] for p in lps])]).astype(np.int64)
    co = np.concatenate([[0], np.cumsum([p[0].shape[1] for p in lps])]).astype(np.int64)
    vecs = [np.ascontiguousarray(np.concatenate([p[q] for p in lps])) for q in (1, 2, 3, 4)]
    return A, ro, co, vecs


def load_batch(kkt, nlp, ro, co, vecs):
    ptr = lambda a: None if a is None else _lib.as_pd(a)         # noqa: E731
    rc = _lib.lib().tlpk_ipm_load_batch(kkt._h, nlp, None if ro is None else _lib.as_p64(ro), None if co is None else _lib.as_p64(co), *[ptr(v) for v in vecs])
    return rc, _lib.lib().tlpk_last_error(kkt._h).decode()


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_batch_symbols_are_declared_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "tlpk.h")).read()
    L = _lib.lib()
    for name in BATCH_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name


def test_load_batch_checks_its_arguments_in_order():
    A, ro, co, vecs = stacked_handle()
    m, n = A.shape
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=-1, row_block=np.repeat(np.arange(3), np.diff(ro))))
    bad = lambda *a: load_batch(kkt, *a)                          # noqa: E731
    rc, msg = bad(3, ro, co, [None] + vecs[1:]); assert rc == _lib.BADARG and "NULL" in msg
    rc, msg = bad(3, None, co, vecs); assert rc == _lib.BADARG and "NULL" in msg
    rc, msg = bad(0, ro, co, vecs); assert rc == _lib.BADARG and "nlp" in msg
    short = ro.copy(); short[-1] -= 1
    rc, msg = bad(3, short, co, vecs); assert rc == _lib.BADARG and "end at m" in msg
    shortc = co.copy(); shortc[-1] += 1
    rc, msg = bad(3, ro, shortc, vecs); assert rc == _lib.BADARG and "end at m" in msg
    dec = ro.copy(); dec[1], dec[2] = ro[2], ro[1]
    rc, msg = bad(3, dec, co, vecs); assert rc == _lib.BADARG and "decrease" in msg
    empty = co.copy(); empty[1] = co[0]
    rc, msg = bad(3, ro, empty, vecs); assert rc == _lib.BADARG and "empty segment" in msg
    # the argument checks come before the device check: a clean call on this analyse-only handle
    rc, msg = bad(3, ro, co, vecs); assert rc == _lib.NO_DEVICE
    kkt.close()
    # one entry moved outside its diagonal block (row 0 of LP 0 into the first column of LP 1), K1 and K2
    Ab = A.tolil(); Ab[0, co[1]] = 1.5; Ab = Ab.tocsc()
    for system in (tk.K1(), tk.K2()):
        kkt = tk.setup(Ab, system, tk.Backend(device=-1))
        rc, msg = load_batch(kkt, 3, ro, co, vecs)
        assert rc == _lib.BADARG and "outside the diagonal block" in msg, msg
        kkt.close()
        kkt = tk.setup(A, system, tk.Backend(device=-1))
        assert load_batch(kkt, 3, ro, co, vecs)[0] == _lib.NO_DEVICE
        kkt.close()


def test_load_batch_refuses_handles_it_cannot_drive_and_the_calls_need_a_load():
    A, ro, co, vecs = stacked_handle()
    L = _lib.lib()
    for kkt, word in ((tk.setup(A, tk.K1(), tk.KrylovBackend(device=-1)), "Krylov"),
                      (tk.setup(A, tk.K2(), tk.KrylovBackend(device=-1, method="minres")), "Krylov"),
                      (tk.setup(A, tk.K1(), tk.Backend(device=-1, dense_cols=[0, 8])), "dense columns"),
                      (tk.setup(A.toarray(), tk.K1(), tk.DenseBackend(device=-1)), "dense-matrix")):
        if word == "dense columns":
            assert kkt.stats()["n_dense_cols"] == 2
        rc, msg = load_batch(kkt, 3, ro, co, vecs)
        assert rc == _lib.BADARG and word in msg, (word, msg)
        kkt.close()
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=-1))
    assert load_batch(kkt, 3, ro, co, vecs)[0] == _lib.NO_DEVICE
    act = np.ones(3, dtype=np.uint8); d = np.ones(64); fail = C.c_int64(7)
    pa, pd_ = _lib.as_pu8(act), _lib.as_pd(d)
    calls = [lambda: L.tlpk_ipm_batch_residuals(kkt._h, pd_, pd_), lambda: L.tlpk_ipm_batch_factor(kkt._h, pa, pd_, pd_, C.byref(fail)),
             lambda: L.tlpk_ipm_batch_hsolve_newton(kkt._h, pa, pd_, pd_), lambda: L.tlpk_ipm_batch_newton(kkt._h, 0, pa, pd_, pd_),
             lambda: L.tlpk_ipm_batch_targets(kkt._h, pa, pd_, pd_), lambda: L.tlpk_ipm_batch_accept(kkt._h, pa),
             lambda: L.tlpk_ipm_batch_advance(kkt._h, pa, pd_, pd_)]
    for call in calls:
        assert call() == _lib.BADARG
        assert b"load first" in L.tlpk_last_error(kkt._h)
    assert L.tlpk_ipm_batch_residuals(None, pd_, pd_) == _lib.BADARG
    kkt.close()


def test_batched_loop_stacks_the_lps():
    lps = small_lps()
    opt = BatchedDeviceHSD(lps, device=-1, load=False)
    assert opt.nlp == 3 and (opt.m, opt.n) == (10, 20)
    assert opt.row_off.tolist() == [0, 3, 8, 10] and opt.col_off.tolist() == [0, 7, 16, 20]
    assert opt.row_block.tolist() == [0] * 3 + [1] * 5 + [2] * 2
    assert np.array_equal(opt.kkt.backend_options.row_block, opt.row_block)
    assert (opt.A != sp.block_diag([p[0] for p in lps])).nnz == 0
    for k, (A, b, c, l, u) in enumerate(lps):
        lf, uf = np.isfinite(l), np.isfinite(u)
        assert opt.p[k] == lf.sum() + uf.sum()
        assert opt.nb[k] == np.abs(b).max() and opt.nc[k] == np.abs(c).max()
        assert opt.nlz[k] == np.abs(np.where(lf, l, 0.0)).max() and opt.nuz[k] == np.abs(np.where(uf, u, 0.0)).max()
        assert np.array_equal(opt._b[opt.row_off[k]:opt.row_off[k + 1]], b) and np.array_equal(opt._u[opt.col_off[k]:opt.col_off[k + 1]], u)
    with pytest.raises(RuntimeError, match="nothing is loaded"):
        opt.optimize()
    with pytest.raises(tk.DimensionMismatch):
        BatchedDeviceHSD([lps[0][:1] + (np.ones(9),) + lps[0][2:]], device=-1, load=False)
    with pytest.raises(ValueError, match="single-device"):
        BatchedDeviceHSD(lps, device=-1, load=False, ngpus=2)
    # a list of standard_form results works directly, K2 as well
    opt2 = BatchedDeviceHSD([golden("lpex_opt"), golden("lpex_freevars")], system="K2", device=-1, load=False)
    assert opt2.nlp == 2 and tk.linear_system(opt2.kkt) == "Augmented system (K2)"
    opt.kkt.close(); opt2.kkt.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------------
def single(d, system="K1", options=None, **kw):
    """One LP through its own DeviceHSD: the record the batch is held to."""
    opt = DeviceHSD(d.A, d.b, d.c, d.l, d.u, c0=d.c0, objsense_min=d.objsense, device=0, system=system, options=options, **kw).optimize()
    rec = dict(status=opt.status, niter=opt.niter, zp=opt.primal_objective, zd=opt.dual_objective, rho=opt.rho, timers=dict(opt.timers),
               x=opt._get(0, opt.n), y=opt._get(5, opt.m), zl=opt._get(3, opt.n))
    opt.kkt.close()
    return rec


def of_batch(opt, k):
    return dict(status=str(opt.status[k]), niter=int(opt.niter[k]), zp=float(opt.primal_objective[k]), zd=float(opt.dual_objective[k]),
                rho=tuple(opt.rho[k]), timers=opt.timers_of(k), x=opt._get(k, 0), y=opt._get(k, 5), zl=opt._get(k, 3))


def close_to(a, b, obj_tol, vec_tol, niter_tol=0):
    print(f"  {a['status']:22s} niter {a['niter']:3d} / {b['niter']:3d}  zp {a['zp']:.12e} / {b['zp']:.12e}  "
          + "  ".join(f"|d{k}| {np.abs(a[k] - b[k]).max() / max(1.0, np.abs(b[k]).max()):.2e}" for k in ("x", "y", "zl")))
    assert a["status"] == b["status"]
    assert abs(a["niter"] - b["niter"]) <= niter_tol
    assert abs(a["zp"] - b["zp"]) <= obj_tol * (1 + abs(b["zp"])) and abs(a["zd"] - b["zd"]) <= obj_tol * (1 + abs(b["zd"]))
    for k in ("x", "y", "zl"):
        assert np.abs(a[k] - b[k]).max() <= vec_tol * max(1.0, np.abs(b[k]).max()), k


_cache = {}


def example_runs(system):
    """The four example LPs: their standard forms and their own DeviceHSD records (computed once per system, never modified)."""
    if system not in _cache:
        ds = [golden(name) for name in EXAMPLES]
        _cache[system] = (ds, [single(d, system) for d in ds])
    return _cache[system]


def check_lpex_opt(opt, k, system):
    ds, recs = example_runs(system)
    close_to(of_batch(opt, k), recs[0], 1e-9, 1e-6 if system == "K1" else 1e-5)
    assert opt.status[k] == "Trm_Optimal"
    assert abs(opt.solution(k)["z_primal"] - 1.5) <= 100 * SQRT_EPS


@pytest.mark.gpu
@pytest.mark.parametrize("system", ["K1", "K2"])
def test_a_batch_of_one_is_the_unbatched_loop_bit_for_bit(system):
    from test_ipm_harness import random_feasible_lp
    d = standard_form(random_feasible_lp(300, 700, 5, ineq=True))
    rb = np.zeros(d.A.shape[0], dtype=np.int64)                    # the batch's default row_block, given to both
    one = single(d, system, row_block=rb)
    opt = BatchedDeviceHSD([d], system=system, device=0).optimize()
    b = of_batch(opt, 0)
    print(system, one["status"], one["niter"], b["niter"], one["timers"], b["timers"])
    assert one["status"] == "Trm_Optimal", "bad test input"
    assert b["status"] == one["status"] and b["niter"] == one["niter"]
    assert b["timers"]["n_update"] == one["timers"]["n_update"] and b["timers"]["n_solve"] == one["timers"]["n_solve"]
    assert b["zp"] == one["zp"] and b["zd"] == one["zd"]
    assert np.array_equal(b["x"], one["x"]) and np.array_equal(b["y"], one["y"])
    opt.kkt.close()


@pytest.mark.gpu
@pytest.mark.parametrize("system", ["K1", "K2"])
def test_mixed_outcomes_in_one_batch(system):
    ds, recs = example_runs(system)
    opt = BatchedDeviceHSD(ds, system=system, device=0).optimize()
    vtol = 1e-6 if system == "K1" else 1e-5
    for k, name in enumerate(EXAMPLES):
        print(system, name)
        assert recs[k]["status"] == EXAMPLE_STATUS[k], "bad test input"
        close_to(of_batch(opt, k), recs[k], 1e-9, vtol)
    check_lpex_opt(opt, 0, system)
    assert not opt.active.any()
    opt.kkt.close()


def boundary_lps():
    """Segment boundaries: 1 x 1; IPM_T and IPM_T + 1 columns (one block / two blocks of a column kernel); 8 k + 1 rows (a row group of the 8-lane
    row kernel with one live row); and an LP of more than one block in every kernel."""
    from test_ipm_harness import random_feasible_lp
    tiny = LP(sp.csc_matrix(np.array([[1.0]])), np.array([1.0]), 0.0, np.array([1.0]), np.array([1.0]), np.array([0.0]), np.array([np.inf]))
    lps = [tiny, random_feasible_lp(60, 256, 21), random_feasible_lp(70, 257, 22), random_feasible_lp(81, 200, 23), random_feasible_lp(300, 700, 5, ineq=False)]
    ds = [standard_form(lp) for lp in lps]
    assert [d.A.shape for d in ds] == [(1, 1), (60, 256), (70, 257), (81, 200), (300, 700)]
    return ds


def boundary_runs():
    if "boundary" not in _cache:
        ds = boundary_lps()
        _cache["boundary"] = (ds, [single(d) for d in ds])
    return _cache["boundary"]


def batch_records(ds, **kw):
    opt = BatchedDeviceHSD(ds, device=0, **kw).optimize()
    recs = [of_batch(opt, k) for k in range(len(ds))]
    opt.kkt.close()
    return recs


@pytest.mark.gpu
def test_segment_boundaries():
    ds, recs = boundary_runs()
    for r in recs:
        assert r["status"] == "Trm_Optimal", "bad test input"
    got = _cache["boundary_batch"] = batch_records(ds)
    for k in range(len(ds)):
        close_to(got[k], recs[k], 1e-8, 1e-6, niter_tol=1)


@pytest.mark.gpu
def test_batches_are_deterministic_and_independent_of_their_composition():
    ds, recs = boundary_runs()
    first = _cache.get("boundary_batch") or batch_records(ds)
    again = batch_records(ds)
    for a, b in zip(first, again):
        assert a["status"] == b["status"] and a["niter"] == b["niter"] and a["zp"] == b["zp"] and a["zd"] == b["zd"] and a["rho"] == b["rho"]
        assert a["timers"] == b["timers"]
        for k in ("x", "y", "zl"):
            assert np.array_equal(a[k], b[k]), k
    order = [3, 0, 4, 2, 1]
    shuffled = batch_records([ds[k] for k in order])
    for pos, k in enumerate(order):
        close_to(shuffled[pos], first[k], 1e-8, 1e-6, niter_tol=1)


@pytest.mark.gpu
def test_the_retry_loop_is_per_lp():
    from helpers import check_retry_run
    from test_lp_configs import BUMP_OPT, STAIR25_OPT
    ds = [golden("bump"), golden("lpex_opt"), golden("stair25")]
    opt = BatchedDeviceHSD(ds, device=0).optimize()
    print({k: (opt.status[k], int(opt.niter[k]), opt.timers_of(k)) for k in range(3)})
    sb = opt.solution(0)
    check_retry_run(opt.timers_of(0), sb["status"], sb["z_primal"], BUMP_OPT)
    assert opt.timers_of(1)["n_bump"] == 0
    check_lpex_opt(opt, 1, "K1")
    ss = opt.solution(2)
    assert ss["status"] == "Trm_Optimal"
    assert abs(ss["z_primal"] - STAIR25_OPT) <= 1e-6 * (1 + abs(STAIR25_OPT)) and abs(ss["z_dual"] - STAIR25_OPT) <= 1e-6 * (1 + abs(STAIR25_OPT))
    assert abs(ss["z_primal"] - ss["z_dual"]) <= 1e-7 * (1 + abs(ss["z_primal"]))
    assert max(ss["rho"]) <= SQRT_EPS
    opt.kkt.close()


@pytest.mark.gpu
def test_a_failed_lp_does_not_sink_the_batch():
    from test_ipm_harness import random_feasible_lp

    class TwoIterations(Options):
        IterationsLimit = 2

    d = standard_form(random_feasible_lp(81, 200, 23))
    ds, recs = example_runs("K1")
    opt = BatchedDeviceHSD([d, ds[0]], options=[TwoIterations(), Options()], device=0).optimize()
    assert opt.status[0] == "Trm_IterationLimit" and opt.niter[0] == 2
    check_lpex_opt(opt, 1, "K1")
    assert opt.niter[1] > 2 and opt.timers_of(1)["n_update"] > opt.timers_of(0)["n_update"] == 2
    assert opt.last_update_rc == _lib.OK                           # the updates after LP 0 left ran with its block parked
    opt.kkt.close()


@pytest.mark.gpu
def test_reload_equals_a_fresh_batch():
    ds, _ = example_runs("K1")
    ds = [ds[0], ds[3], standard_form(read_free_mps(os.path.join(GOLDEN, "stair25.mps")))]
    opt = BatchedDeviceHSD(ds, device=0).optimize()
    rng = np.random.default_rng(3)
    c2 = opt._c * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, opt.n))
    opt.reload(c=c2).optimize()
    fresh = BatchedDeviceHSD([(d.A, d.b, c2[opt.col_off[k]:opt.col_off[k + 1]], d.l, d.u, d.c0, d.objsense) for k, d in enumerate(ds)], device=0).optimize()
    for k in range(3):
        a, b = of_batch(opt, k), of_batch(fresh, k)
        assert a["status"] == b["status"] and a["niter"] == b["niter"] and a["zp"] == b["zp"] and a["zd"] == b["zd"] and a["timers"] == b["timers"]
        for key in ("x", "y", "zl"):
            assert np.array_equal(a[key], b[key]), key
    assert opt.status[0] == "Trm_Optimal"
    opt.kkt.close(); fresh.kkt.close()


@pytest.mark.gpu
def test_model_optimize_batch():
    paths = [os.path.join(GOLDEN, name + ".mps") for name in EXAMPLES]
    own = [tk.Model.load(p, device=0).optimize() for p in paths]
    models = tk.Model.optimize_batch([tk.Model.load(p) for p in paths], device=0)
    print([(m.status, m.inner is None) for m in own])
    for a, b in zip(models, own):
        assert a.status == b.status
        assert (a.inner is None) == (b.inner is None)            # (a model presolve alone solves never reaches the batch)
        for f in ("objective_value", "dual_objective_value"):
            za, zb = getattr(a, f)(), getattr(b, f)()
            assert (za == zb) or abs(za - zb) <= 1e-9 * (1 + abs(zb)), (f, za, zb)
    assert [m.status for m in own] == EXAMPLE_STATUS


@pytest.mark.gpu
def test_batched_and_unbatched_calls_refuse_each_other():
    A, ro, co, vecs = stacked_handle()
    L = _lib.lib()
    out = np.zeros(64); tau = np.ones(3)
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=0))
    assert load_batch(kkt, 3, ro, co, vecs)[0] == _lib.OK
    assert L.tlpk_ipm_residuals(kkt._h, 1.0, _lib.as_pd(out)) == _lib.BADARG
    assert b"tlpk_ipm_batch" in L.tlpk_last_error(kkt._h)
    assert L.tlpk_ipm_factor(kkt._h, 1.0, 1.0) == _lib.BADARG and L.tlpk_mpc_start(kkt._h, _lib.as_pd(out)) == _lib.BADARG
    assert L.tlpk_ipm_load(kkt._h, *[_lib.as_pd(v) for v in vecs]) == _lib.BADARG
    assert load_batch(kkt, 3, ro, co, vecs)[0] == _lib.BADARG
    assert L.tlpk_ipm_batch_residuals(kkt._h, _lib.as_pd(tau), _lib.as_pd(out)) == _lib.OK
    assert L.tlpk_ipm_reset(kkt._h) == _lib.OK
    x = np.ones(A.shape[1])
    assert L.tlpk_ipm_get(kkt._h, 0, _lib.as_pd(x), x.shape[0]) == _lib.OK and not x.any()
    kkt.close()
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=0))
    assert L.tlpk_ipm_load(kkt._h, *[_lib.as_pd(v) for v in vecs]) == _lib.OK
    assert L.tlpk_ipm_batch_residuals(kkt._h, _lib.as_pd(tau), _lib.as_pd(out)) == _lib.BADARG
    assert b"tlpk_ipm_load_batch" in L.tlpk_last_error(kkt._h)
    assert load_batch(kkt, 3, ro, co, vecs)[0] == _lib.BADARG
    assert L.tlpk_ipm_residuals(kkt._h, 1.0, _lib.as_pd(out)) == _lib.OK
    kkt.close()
