"""Per-LP pivot verdicts and the retry of the failed LPs alone (`tlpk_ipm_batch_factor_each`; `BatchedDeviceHSD / BatchedDeviceMPC(retry="failed")`,
tulip_jl_amd/batch_retry.py; DESIGN.md section 4b'-v).

CPU: the ABI surface; the refusals of the call on handles without a load; the retry loop against a stub update -- random failure patterns, LPs that
reach three bumps, several LPs failing in one round: `"failed"` ends with the regularisations, bump counts and statuses of `"all"`, never makes
more calls, and never factorises an LP again that holds a factor.

GPU (K1, K2): a stacked handle whose blocks are one front each of every class of diagonal-block kernel (the boundaries of tlpk_host.hpp /
schedule.cpp: an isolated 1 x 1 front; ns = 2 <= SMALL_NS, one wave; ns = 65 > NB_IN, the 64-block kernels; ns = 257 > 256, two outer block columns,
in launch form and, with TLPK_CHAIN=1, in chain form) gets a verdict per LP that the existing call confirms one LP at a time; a hold keeps every bit;
the two loops end bit-identical under both `retry` settings with fewer update calls; an LP's run does not depend on its neighbours.  Under K2 the
four columns of bump.mps without entries are isolated nodes that the analysis gathers, for all copies, in ONE root front: the front the holds admit
as shared (it stands alone and is factorised by every call)."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import tulip_jl_amd as tk
from test_hsd_batch import GOLDEN, ROOT, golden, load_batch, stacked_handle
from tulip_jl_amd import _lib
from tulip_jl_amd.batch_retry import factor_failed
from tulip_jl_amd.hsd_batch import BatchedDeviceHSD
from tulip_jl_amd.hsd_device import DeviceHSD, Options
from tulip_jl_amd.mpc_batch import BatchedDeviceMPC

pu8, pd, p64 = _lib.as_pu8, _lib.as_pd, _lib.as_p64
NAME = "tlpk_ipm_batch_factor_each"


def last_error(h):
    return _lib.lib().tlpk_last_error(h).decode()


def bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def each(h, role, regP, regD):
    """One tlpk_ipm_batch_factor_each: (rc, fail_col, nfail)."""
    role = np.ascontiguousarray(role, dtype=np.uint8)
    fail_col = np.full(role.shape[0], -7, dtype=np.int64)
    nfail = C.c_int64(-7)
    rc = _lib.lib().tlpk_ipm_batch_factor_each(h, pu8(role), pd(np.ascontiguousarray(regP)), pd(np.ascontiguousarray(regD)), p64(fail_col), C.byref(nfail))
    return rc, fail_col, int(nfail.value)


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_call_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "tlpk.h")).read()
    L = _lib.lib()
    assert hasattr(L, NAME), NAME                                          # (without the feature the file fails here: the symbol is missing)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", header)
    assert NAME in _lib.EXPORTS
    assert getattr(L, NAME).restype is C.c_int and len(getattr(L, NAME).argtypes) == 6
    assert not NAME.startswith(("tlpk_update", "tlpk_solve", "tlpk_refine", "tlpk_root", "tlpk_sync"))      # tests/test_api_contract.py tabulates those


def test_the_call_refuses_in_order_without_a_load():
    """h NULL, then "not batch-loaded" before everything else.  Nothing can be loaded without a device (tlpk_ipm_load_batch answers TLPK_NO_DEVICE on
    an analyse-only handle), so on this machine every call on a handle ends at the second refusal -- the valid one included; the refusals behind it (a
    NULL pointer, a role above 3, the stale handle, the hold on refine_steps > 0) need a loaded handle and are checked on the GPU
    (test_the_refusals_behind_the_load); TLPK_NO_DEVICE behind them cannot be reached by any handle: one without a device is never loaded."""
    A, ro, co, vecs = stacked_handle()
    L = _lib.lib()
    role, d = np.array([1, 0, 2], dtype=np.uint8), np.ones(3)
    fc, nf = np.zeros(3, dtype=np.int64), C.c_int64(0)
    assert L.tlpk_ipm_batch_factor_each(None, pu8(role), pd(d), pd(d), p64(fc), C.byref(nf)) == _lib.BADARG
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=-1, row_block=np.repeat(np.arange(3), np.diff(ro))))
    assert load_batch(kkt, 3, ro, co, vecs)[0] == _lib.NO_DEVICE
    bad_role = np.array([1, 4, 0], dtype=np.uint8)
    for args in ((pu8(role), pd(d), pd(d), p64(fc), C.byref(nf)),            # valid
                 (None, pd(d), pd(d), p64(fc), C.byref(nf)), (pu8(role), None, pd(d), p64(fc), C.byref(nf)), (pu8(role), pd(d), None, p64(fc), C.byref(nf)),
                 (pu8(role), pd(d), pd(d), None, C.byref(nf)), (pu8(role), pd(d), pd(d), p64(fc), None),
                 (pu8(bad_role), pd(d), pd(d), p64(fc), C.byref(nf))):
        assert L.tlpk_ipm_batch_factor_each(kkt._h, *args) == _lib.BADARG and "load first" in last_error(kkt._h)
    kkt.close()


class StubLoop:
    """What batch_retry.factor_failed and BatchedDeviceHSD._factor need of their owner, with an update that fails by a per-LP script: LP k fails its
    first need[k] updates (an update factorises LP k with the regularisations it has then, so the script counts the LP's bumps)."""
    _bumped = ("regD", "regP", "regG")
    _factor = BatchedDeviceHSD._factor
    _factor_enter = BatchedDeviceMPC._factor_enter
    retry = "all"

    def __init__(self, need, order, enter_fails=None):
        B = self.nlp = len(need)
        self.enter_fails = np.zeros(B, dtype=bool) if enter_fails is None else np.asarray(enter_fails)      # an entering LP's starting matrix fails, whatever is bumped
        self.evicted = []
        self.need, self.order = np.asarray(need), np.asarray(order)         # order: the permuted column an LP's failure is reported at (the smallest wins in `all`)
        self.regP, self.regD, self.regG = np.full(B, 1e-3), np.full(B, 2e-3), np.full(B, 3e-3)
        self.status = np.array(["Trm_Unknown"] * B, dtype=object)
        self.timers = {name: np.zeros(B, dtype=np.int64) for name in ("n_update", "n_bump", "max_bumps_in_a_step")}
        self.timers["n_update_calls"] = self.timers["n_lp_factor"] = 0
        self.bump_log, self.last_update_rc = [], None
        self.factorised = []                                                 # per call: the LPs it factorised
        self.kkt = type("H", (), {"_h": None})()
        self.L = self

    def _fails(self, k):
        return int(round(np.log(self.regD[k] / 2e-3) / np.log(100.0))) < self.need[k]

    # retry="all": the library call
    def tlpk_ipm_batch_factor(self, h, active, regP, regD, fail):
        act = np.ctypeslib.as_array(active, shape=(self.nlp,)).astype(bool)
        self.factorised.append(act.copy())
        bad = [k for k in np.flatnonzero(act) if self._fails(k)]
        if not bad:
            return _lib.OK
        fail._obj.value = min(bad, key=lambda k: self.order[k])
        return _lib.NOT_POSDEF

    def tlpk_mpc_batch_factor_enter(self, h, active, enter, regP, regD, fail):
        act = np.ctypeslib.as_array(active, shape=(self.nlp,)).astype(bool)
        ent = np.ctypeslib.as_array(enter, shape=(self.nlp,)).astype(bool)
        assert not (act & ent).any()
        self.factorised.append(act | ent)
        bad = [k for k in np.flatnonzero(act) if self._fails(k)] + [k for k in np.flatnonzero(ent) if self.enter_fails[k]]
        if not bad:
            return _lib.OK
        fail._obj.value = min(bad, key=lambda k: self.order[k])
        return _lib.NOT_POSDEF

    def _evict(self, k):
        self.evicted.append(int(k))

    def _last_error(self):
        return ""

    def _mask(self, m):
        self._m8 = np.ascontiguousarray(m, dtype=np.uint8)
        return pu8(self._m8)

    # retry="failed": the callable
    def each(self, role):
        work = (role == 1) | (role == 3)
        self.factorised.append(work.copy())
        self.roles.append(role.copy())
        fail_col = np.full(self.nlp, -1, dtype=np.int64)
        for k in np.flatnonzero(work):
            if (self._fails(k) if role[k] == 1 else self.enter_fails[k]):
                fail_col[k] = self.order[k]
        self.failed.append(fail_col >= 0)
        return (_lib.NOT_POSDEF if (fail_col >= 0).any() else _lib.OK), fail_col

    roles = failed = None

    def _call(self, rc):
        raise AssertionError(rc)


def test_the_retry_loop_against_a_stub_update():
    rng = np.random.default_rng(20261020)
    seen_three, seen_multi = 0, 0
    for trial in range(200):
        B = int(rng.integers(1, 9))
        need = rng.choice([0, 0, 0, 1, 1, 2, 3, 4], size=B)                  # 3, 4: the LP reaches three bumps and is out
        order = rng.permutation(B) * 10 + 3
        step = rng.random(B) < 0.85
        if not step.any():
            step[0] = True
        a, f = StubLoop(need, order), StubLoop(need, order)
        f.roles, f.failed = [], []
        held_a = a._factor(step)
        held_f, _ = factor_failed(f, step, np.zeros(B, dtype=bool), f.each)
        assert np.array_equal(held_a, held_f), trial
        for name in ("regP", "regD", "regG"):
            assert bits(getattr(a, name), getattr(f, name)), (trial, name)
        assert list(a.status) == list(f.status), trial
        for name in ("n_update", "n_bump", "max_bumps_in_a_step"):
            assert np.array_equal(a.timers[name], f.timers[name]), (trial, name)
        assert len(a.bump_log) == len(f.bump_log) and all(np.array_equal(x, y) for x, y in zip(a.bump_log, f.bump_log)), trial
        expect_gone = step & (need >= 3)
        assert np.array_equal(f.status == "Trm_NumericalProblem", expect_gone) and np.array_equal(held_f, step & ~expect_gone), trial
        assert f.timers["n_update_calls"] <= a.timers["n_update_calls"], trial
        assert f.timers["n_update_calls"] == len(f.factorised) and a.timers["n_update_calls"] == len(a.factorised)
        assert f.timers["n_lp_factor"] == sum(int(w.sum()) for w in f.factorised) <= a.timers["n_lp_factor"] == sum(int(w.sum()) for w in a.factorised)
        # the rounds: every LP of `step` in the first, afterwards only LPs that failed the round before; an LP that came through holds from then on, an
        # LP that is out or was never in the step is parked; the last call (if any LP is left) returned TLPK_OK
        ok = np.zeros(B, dtype=bool)
        for r, role in enumerate(f.roles):
            if r == 0:
                assert np.array_equal(role == 1, step) and not (role == 2).any()
            assert not (ok & (role == 1)).any(), (trial, r)                  # a held LP is never active again within the pass
            assert np.array_equal(role == 2, ok), (trial, r)
            if r > 0:
                assert not ((role == 1) & ~f.failed[r - 1]).any(), (trial, r)
            ok |= (role == 1) & ~f.failed[r]
        if held_f.any():
            assert f.last_update_rc == _lib.OK
        if (step & (need > 0)).sum() >= 2:
            seen_multi += 1
            if (step & (need > 0) & (need < 3)).sum() >= 2 and len(set(need[step & (need > 0)])) == 1:
                assert f.timers["n_update_calls"] < a.timers["n_update_calls"], trial      # K LPs with the same need: K (need) + 1 calls against need + 1
        seen_three += int(expect_gone.any())
    assert seen_three > 20 and seen_multi > 50                               # the patterns the loop is for were drawn


class StubMPC(StubLoop):
    _bumped = ("regD", "regP")


def test_the_retry_loop_with_entering_lps_against_a_stub_update():
    """Role 3: entering LPs ride in the update of the active ones (the Mehrotra stream).  An entering LP with a verdict is out at once, evicted, and not
    bumped; its neighbours that came through hold; `"failed"` ends as `"all"` (`_factor_enter`) does."""
    rng = np.random.default_rng(20261021)
    seen_enter_fail, seen_mixed, fewer = 0, 0, 0
    for trial in range(300):
        B = int(rng.integers(2, 9))
        need = rng.choice([0, 0, 0, 1, 1, 2, 3], size=B)
        order = rng.permutation(B) * 10 + 3
        kind = rng.choice([0, 1, 2], size=B, p=[0.15, 0.55, 0.3])              # parked, active, entering
        step, enter = kind == 1, kind == 2
        if not enter.any():
            enter[0], step[0] = True, False
        enter_fails = enter & (rng.random(B) < 0.4)
        a, f = StubMPC(need, order, enter_fails), StubMPC(need, order, enter_fails)
        f.roles, f.failed = [], []
        sa, ea = a._factor_enter(step, enter)
        sf, ef = factor_failed(f, step, enter, f.each)
        assert np.array_equal(sa, sf) and np.array_equal(ea, ef), trial
        assert np.array_equal(ef, enter & ~enter_fails) and np.array_equal(sf, step & (need < 3)), trial
        for name in ("regP", "regD", "regG"):
            assert bits(getattr(a, name), getattr(f, name)), (trial, name)
        assert bits(f.regG, np.full(B, 3e-3)) and bits(f.regD[enter], np.full(int(enter.sum()), 2e-3))      # MPC bumps no regG; an entering LP is never bumped
        assert list(a.status) == list(f.status) and sorted(a.evicted) == sorted(f.evicted) == np.flatnonzero(enter_fails).tolist(), trial
        for name in ("n_update", "n_bump", "max_bumps_in_a_step"):
            assert np.array_equal(a.timers[name], f.timers[name]), (trial, name)
        assert len(a.bump_log) == len(f.bump_log) and all(np.array_equal(x, y) for x, y in zip(a.bump_log, f.bump_log)), trial
        assert f.timers["n_update_calls"] <= a.timers["n_update_calls"] and f.timers["n_lp_factor"] <= a.timers["n_lp_factor"], trial
        ok = np.zeros(B, dtype=bool)
        for r, role in enumerate(f.roles):
            if r == 0:
                assert np.array_equal(role == 1, step) and np.array_equal(role == 3, enter) and not (role == 2).any()
            else:
                assert not (role == 3).any(), (trial, r)                     # an entering LP either came through (hold) or is out (parked)
                assert not ((role == 1) & ~f.failed[r - 1]).any(), (trial, r)
            assert not (ok & ((role == 1) | (role == 3))).any() and np.array_equal(role == 2, ok), (trial, r)
            ok |= ((role == 1) | (role == 3)) & ~f.failed[r]
        if sf.any() or ef.any():
            assert f.last_update_rc == _lib.OK
        seen_enter_fail += int(enter_fails.any())
        seen_mixed += int(enter_fails.any() and (step & (need > 0)).any())
        fewer += int(f.timers["n_update_calls"] < a.timers["n_update_calls"])
    assert seen_enter_fail > 50 and seen_mixed > 30 and fewer > 50


def test_python_passes_retry_through_and_checks_it():
    with pytest.raises(ValueError, match="retry"):
        BatchedDeviceHSD([golden("lpex_opt")], device=-1, load=False, retry="some")
    opt = BatchedDeviceMPC([golden("lpex_opt")], device=-1, load=False, retry="failed")
    assert opt.retry == "failed" and opt.timers["n_update_calls"] == 0 and "n_update_calls" not in opt.timers_of(0)
    with pytest.raises(ValueError, match="retry"):
        opt.optimize_stream([], retry="none")
    opt.kkt.close()
    paths = [os.path.join(GOLDEN, "lpex_opt.mps")] * 2
    with pytest.raises(ValueError, match="retry"):
        tk.Model.optimize_stream([tk.Model.load(p) for p in paths], 2, device=-1, retry="x")


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the call
# ---------------------------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 2), (2, 3), (65, 70), (257, 260), (3, 5), (4, 6)]              # dense blocks: S_k (K1) is dense, one front of ns = rows
F = [0, 1, 2, 3]                                                            # one LP per kernel class gets the bad values; LPs 4 and 5 never do
CASES = [("K1", "0"), ("K1", "1"), ("K2", "0"), ("K2", "1")]
CASE_IDS = [f"{s}-{'chain' if c == '1' else 'launch'}" for s, c in CASES]


def class_lps():
    rng = np.random.default_rng(5)
    out = []
    for (m, n) in SIZES:
        A = sp.csc_matrix(rng.standard_normal((m, n)))
        out.append((A, np.ones(m), np.ones(n), np.zeros(n), np.full(n, np.inf)))
    return out


def class_handle(system, chain, monkeypatch, **kw):
    """The stacked handle, batch-loaded (the iterate is the starting point), with the proof that every kernel class is in its schedule."""
    monkeypatch.setenv("TLPK_CHAIN", chain)
    monkeypatch.setenv("TLPK_POISON", "1")                                  # panel storage that no kernel writes holds the same bits on every handle (two are compared)
    A, ro, co, vecs = stacked_handle(class_lps())
    kkt = tk.setup(A, tk.K2() if system == "K2" else tk.K1(), tk.Backend(device=0, row_block=np.repeat(np.arange(len(SIZES)), np.diff(ro)), **kw))
    rc, msg = load_batch(kkt, len(SIZES), ro, co, vecs)
    assert rc == _lib.OK, msg
    ns = kkt.symbolic("front_ns")
    potrf = kkt.symbolic("potrf_tasks").reshape(-1, 4)
    nsingle = (kkt.symbolic("singles").size - 2) // 3
    nchain = kkt.symbolic("chain_items").size
    if system == "K1":
        assert sorted(ns.tolist()) == sorted(m for m, _ in SIZES) and nsingle == 1      # one front per block; the 1 x 1 block is an isolated front
    else:
        assert len(ns) == len(SIZES) and nsingle == 0                       # (an augmented system has no isolated node: every variable meets a constraint)
    assert (ns <= 16).any() and ((ns > 64) & (ns <= 256)).any() and (ns > 256).any()    # one wave | the 64-block kernels | more than one 256-wide block column
    assert (potrf[:, 2] > 64).any()                                         # a diagonal block of several 64-wide steps
    assert (nchain > 0) == (chain == "1")                                   # the dependency-driven form of the wide front, or its launches
    return kkt, ro, co


def good(B):
    return np.full(B, 1e-4), np.full(B, 1e-4)


def with_bad(B, ks):
    """A negative regD under a huge regP: S_k = A_k D_k A_k' + regD_k I is negative definite (K2: the constraint nodes' pivots have the wrong sign)."""
    rP, rD = good(B)
    rP[ks] = 1e30
    rD[ks] = -1.0
    return rP, rD


def state(kkt, m, n):
    out = [kkt.factor_panels()]
    for code, length in ((_lib.IPM_THETA, n), (_lib.IPM_REGP, n), (_lib.IPM_REGD, m)):
        v = np.empty(length)
        assert _lib.lib().tlpk_ipm_get(kkt._h, code, pd(v), length) == _lib.OK
        out.append(v)
    return out


def hsolve(kkt, B):
    sc = np.zeros((B, 8)); sc[:, 0] = 1.0; sc[:, 1] = 1.0; sc[:, 2] = 1e-4; sc[:, 4] = -1.0
    out = np.zeros((B, 4))
    act = np.ones(B, dtype=np.uint8)
    assert _lib.lib().tlpk_ipm_batch_hsolve_newton(kkt._h, pu8(act), pd(sc), pd(out)) == _lib.OK
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("system,chain", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("skip", [0, 1], ids=["noskip", "skip"])
def test_a_verdict_at_every_recording_site_and_a_hold_that_keeps_every_bit(system, chain, skip, monkeypatch):
    L = _lib.lib()
    B = len(SIZES)
    kkt, ro, co = class_handle(system, chain, monkeypatch)
    m, n = int(ro[-1]), int(co[-1])
    assert L.tlpk_ipm_batch_skip(kkt._h, skip) == _lib.OK
    ones = np.ones(B, dtype=np.uint8)
    fail = C.c_int64(-1)
    # the yardstick: the existing call, one bad LP at a time
    c_of = {}
    for k in F:
        rP, rD = with_bad(B, [k])
        assert L.tlpk_ipm_batch_factor(kkt._h, pu8(ones), pd(rP), pd(rD), C.byref(fail)) == _lib.NOT_POSDEF
        assert fail.value == k
        c_of[k] = kkt.stats()["fail_col"]
    print(system, chain, "first bad columns", c_of)
    # no failure: the new call is the existing one, bit for bit.  The existing call runs on a SECOND handle, which takes that one all-good update and
    # nothing else; the first handle holds the factor of the failed yardstick calls until the new call replaces every bit of it
    gP, gD = good(B)
    other, _, _ = class_handle(system, chain, monkeypatch)
    assert L.tlpk_ipm_batch_skip(other._h, skip) == _lib.OK
    assert L.tlpk_ipm_batch_factor(other._h, pu8(ones), pd(gP), pd(gD), C.byref(fail)) == _lib.OK and fail.value == -1
    ref = state(other, m, n)
    ref_solve = hsolve(other, B)
    other.close()
    before = state(kkt, m, n)
    assert not bits(before[0], ref[0])                                      # (the panels of the failed updates differ: the next call has work to do)
    rc, fc, nf = each(kkt._h, ones, gP, gD)
    assert rc == _lib.OK and nf == 0 and (fc == -1).all()
    for a, b in zip(state(kkt, m, n), ref):
        assert bits(a, b)
    assert bits(hsolve(kkt, B), ref_solve)
    # every LP of F bad at once
    rP, rD = with_bad(B, F)
    rc, fc, nf = each(kkt._h, ones, rP, rD)
    assert rc == _lib.NOT_POSDEF and nf == len(F)
    assert fc.tolist() == [c_of.get(k, -1) for k in range(B)]
    assert kkt.stats()["fail_col"] == min(c_of.values())
    # the hold: F again with good values, the others keep their factor; their entries of regP / regD are not read
    role = np.full(B, 2, dtype=np.uint8); role[F] = 1
    hP, hD = good(B)
    rest = [k for k in range(B) if k not in F]
    hP[rest] = np.nan; hD[rest] = np.nan
    rc, fc, nf = each(kkt._h, role, hP, hD)
    assert rc == _lib.OK and nf == 0 and (fc == -1).all()
    for a, b in zip(state(kkt, m, n), ref):
        assert bits(a, b)
    assert bits(hsolve(kkt, B), ref_solve)
    assert kkt.symbolic("front_skip").size == 0 or not kkt.symbolic("front_skip").any()      # (no mask of tlpk_block_skip's was left behind)
    kkt.close()


@pytest.mark.gpu
@pytest.mark.parametrize("system", ["K1", "K2"])
def test_verdicts_from_the_older_diagonal_block_kernel(system, monkeypatch):
    """TLPK_POTRF_MODE=0 (re-read at every launch under TLPK_POTRF_DYN): the 64-block kernels run potrf_block, whose recording site is its own."""
    monkeypatch.setenv("TLPK_POTRF_DYN", "1")
    monkeypatch.setenv("TLPK_POTRF_MODE", "0")
    L = _lib.lib()
    B = len(SIZES)
    kkt, ro, co = class_handle(system, "0", monkeypatch)
    ones = np.ones(B, dtype=np.uint8)
    fail = C.c_int64(-1)
    c_of = {}
    for k in F:
        rP, rD = with_bad(B, [k])
        assert L.tlpk_ipm_batch_factor(kkt._h, pu8(ones), pd(rP), pd(rD), C.byref(fail)) == _lib.NOT_POSDEF and fail.value == k
        c_of[k] = kkt.stats()["fail_col"]
    rP, rD = with_bad(B, F)
    rc, fc, nf = each(kkt._h, ones, rP, rD)
    assert rc == _lib.NOT_POSDEF and nf == len(F) and fc.tolist() == [c_of.get(k, -1) for k in range(B)]
    assert kkt.stats()["fail_col"] == min(c_of.values())
    gP, gD = good(B)
    rc, fc, nf = each(kkt._h, ones, gP, gD)
    assert rc == _lib.OK and nf == 0 and (fc == -1).all()
    kkt.close()


@pytest.mark.gpu
def test_the_refusals_behind_the_load(monkeypatch):
    L = _lib.lib()
    B = len(SIZES)
    kkt, ro, co = class_handle("K1", "0", monkeypatch, refine=1)
    gP, gD = good(B)
    ones = np.ones(B, dtype=np.uint8)
    fc, nf = np.zeros(B, dtype=np.int64), C.c_int64(0)
    for args in ((None, pd(gP), pd(gD), p64(fc), C.byref(nf)), (pu8(ones), None, pd(gD), p64(fc), C.byref(nf)), (pu8(ones), pd(gP), None, p64(fc), C.byref(nf)),
                 (pu8(ones), pd(gP), pd(gD), None, C.byref(nf)), (pu8(ones), pd(gP), pd(gD), p64(fc), None)):
        assert L.tlpk_ipm_batch_factor_each(kkt._h, *args) == _lib.BADARG and "NULL pointer" in last_error(kkt._h)
    role = ones.copy(); role[3] = 4
    assert each(kkt._h, role, gP, gD)[0] == _lib.BADARG and "LP 3 has role 4" in last_error(kkt._h)
    role[3] = 2                                                             # a hold on a handle with refine_steps = 1
    assert each(kkt._h, role, gP, gD)[0] == _lib.BADARG and "hold refused: refine_steps" in last_error(kkt._h)
    rc, fcol, nfail = each(kkt._h, ones, gP, gD)                            # ... which stays usable
    assert rc == _lib.OK and nfail == 0
    assert np.isfinite(hsolve(kkt, B)).all()
    # the stale handle: new matrix values after the load (tlpk_set_values) -- behind the role check, and before the hold's conditions
    tk.set_values(kkt, kkt.A.data * 1.5)
    assert each(kkt._h, ones, gP, gD)[0] == _lib.BADARG and "tlpk_ipm_reload" in last_error(kkt._h)
    role[3] = 4
    assert each(kkt._h, role, gP, gD)[0] == _lib.BADARG and "LP 3 has role 4" in last_error(kkt._h)
    role[3] = 2
    assert each(kkt._h, role, gP, gD)[0] == _lib.BADARG and "tlpk_ipm_reload" in last_error(kkt._h)
    kkt.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the loops
# ---------------------------------------------------------------------------------------------------------------------------------------
class Forty(Options):
    IterationsLimit = 40


def bump_copies(B, seed=20261018, rel=0.01):
    """B copies of bump.mps under the seeded cost perturbations of tools/hsd_batch_bench.py (`costs`: dual feasibility is kept)."""
    d = golden("bump")
    lf, uf = np.isfinite(d.l), np.isfinite(d.u)
    scale = rel * np.maximum(np.abs(d.c), np.abs(d.c).mean())
    out = []
    for k in range(B):
        rng = np.random.default_rng(seed + k)
        up, both = rng.uniform(0.0, 1.0, d.c.shape[0]), rng.uniform(-1.0, 1.0, d.c.shape[0])
        c = d.c + scale * np.where(lf & uf, both, np.where(lf, up, np.where(uf, -up, 0.0)))
        out.append((d.A, d.b, c, d.l, d.u, d.c0, d.objsense))
    return out


def record_of(opt, k):
    return dict(status=str(opt.status[k]), niter=int(opt.niter[k]), timers=opt.timers_of(k), regP=float(opt.regP[k]), regD=float(opt.regD[k]),
                regG=float(opt.regG[k]), vec=[opt._get(k, code) for code in range(6)])


def same_record(a, b, label):
    assert a["status"] == b["status"] and a["niter"] == b["niter"] and a["timers"] == b["timers"], (label, a["status"], b["status"], a["timers"], b["timers"])
    for name in ("regP", "regD", "regG"):
        assert bits(a[name], b[name]), (label, name)
    for code, (u, v) in enumerate(zip(a["vec"], b["vec"])):
        assert bits(u, v), (label, code)


_runs = {}


def loop_run(cls, system, retry, B=6):
    """One optimize() of the six bump copies, computed once per setting and shared."""
    key = (cls.__name__, system, retry, B)
    if key not in _runs:
        opt = cls(bump_copies(B), system=system, device=0, options=Forty(), retry=retry).optimize()
        assert opt.retry == retry                                           # (no fall-back happened)
        _runs[key] = dict(recs=[record_of(opt, k) for k in range(B)], calls=int(opt.timers["n_update_calls"]), bump_log=[b.copy() for b in opt.bump_log])
        opt.kkt.close()
    return _runs[key]


# BatchedDeviceMPC: B = 6 and the default seed (20261018) of the perturbations, as for the homogeneous loop -- on the CPU (tests/ipm_harness.py's MPC with
# the dense Cholesky backend, iteration limit 40) these six copies have passes in which two or more LPs fail their update; the test asserts it of its own run
@pytest.mark.gpu
@pytest.mark.parametrize("cls", [BatchedDeviceHSD, BatchedDeviceMPC], ids=["hsd", "mpc"])
@pytest.mark.parametrize("system", ["K1", "K2"])
def test_both_retry_settings_give_the_same_runs_with_fewer_update_calls(cls, system):
    a, f = loop_run(cls, system, "all"), loop_run(cls, system, "failed")
    multi = sum(1 for nb in a["bump_log"] if (nb > 0).sum() >= 2)
    print(cls.__name__, system, "update calls", a["calls"], "->", f["calls"], "| passes with a bump", len(a["bump_log"]), "with two or more failing LPs", multi,
          "| n_bump", [r["timers"]["n_bump"] for r in a["recs"]])
    assert multi >= 1, "no pass of the retry='all' run had two failing LPs: the comparison would be vacuous"
    for k, (ra, rf) in enumerate(zip(a["recs"], f["recs"])):
        same_record(ra, rf, f"LP {k}")
    assert len(a["bump_log"]) == len(f["bump_log"]) and all(np.array_equal(x, y) for x, y in zip(a["bump_log"], f["bump_log"]))
    assert f["calls"] < a["calls"]


@pytest.mark.gpu
def test_a_stream_of_twelve_through_four_slots():
    lps = bump_copies(12)
    out = {}
    for retry in ("all", "failed"):
        opt = BatchedDeviceHSD(lps[:4], device=0, options=Forty(), retry=retry)
        recs = opt.optimize_stream(lps[4:], options=Forty())
        out[retry] = (recs, int(opt.timers["n_update_calls"]), [b.copy() for b in opt.bump_log])
        opt.kkt.close()
    (ra, ca, la), (rf, cf, lf) = out["all"], out["failed"]
    multi = sum(1 for nb in la if (nb > 0).sum() >= 2)
    print("stream: update calls", ca, "->", cf, "| passes with two or more failing LPs", multi)
    assert multi >= 1 and len(ra) == len(rf) == 12
    for i, (a, f) in enumerate(zip(ra, rf)):
        assert a["status"] == f["status"] and a["niter"] == f["niter"] and a["timers"] == f["timers"], i
        assert (a["slot"], a["entered"], a["left"]) == (f["slot"], f["entered"], f["left"]), i
        for key in ("x", "y", "zl", "zu", "xh", "yh"):
            assert bits(a[key], f[key]), (i, key)
    assert cf < ca


@pytest.mark.gpu
@pytest.mark.parametrize("system", ["K1", "K2"])
def test_a_mehrotra_stream_with_entering_lps_under_both_settings(system):
    """Role 3: in BatchedDeviceMPC.optimize_stream an LP that takes a slot ENTERS through the update of the running LPs.  Twelve bump copies and one LP whose
    matrix holds an entry that is not a number (its starting matrix fails whatever happens: it is out at once and evicted) through four slots: every record
    is the same under both settings, bit for bit, with fewer update calls."""
    lps = bump_copies(12)
    A = lps[6][0].copy(); A.data[0] = np.nan
    queue = lps[4:7] + [(A,) + tuple(lps[6][1:])] + lps[7:]
    out = {}
    for retry in ("all", "failed"):
        opt = BatchedDeviceMPC(lps[:4], system=system, device=0, options=Forty(), retry=retry)
        recs = opt.optimize_stream(queue, options=Forty())
        assert opt.retry == retry
        out[retry] = (recs, int(opt.timers["n_update_calls"]), [b.copy() for b in opt.bump_log], opt.refills)
        opt.kkt.close()
    (ra, ca, la, na), (rf, cf, lf, nf) = out["all"], out["failed"]
    multi = sum(1 for nb in la if (nb > 0).sum() >= 2)
    print(system, "mpc stream: update calls", ca, "->", cf, "| passes with two or more failing LPs", multi, "| refills", na, nf,
          "| statuses", [r["status"] for r in ra])
    assert multi >= 1 and len(ra) == len(rf) == 13 and na == nf
    assert ra[7]["status"] == "Trm_NumericalProblem" and ra[7]["niter"] == 0      # the LP that fails as it enters
    assert sum(1 for r in ra if r["entered"] > 1) >= 8                      # LPs did enter beside running ones
    for i, (a, f) in enumerate(zip(ra, rf)):
        assert a.keys() == f.keys()
        for key in a:
            if isinstance(a[key], np.ndarray):
                assert bits(a[key], f[key]) or (i == 7 and np.array_equal(np.isnan(a[key]), np.isnan(f[key]))), (i, key)
            else:
                assert a[key] == f[key] or (isinstance(a[key], float) and bits(a[key], f[key])), (i, key, a[key], f[key])
    assert len(la) == len(lf) and all(np.array_equal(x, y) for x, y in zip(la, lf))
    assert cf < ca


@pytest.mark.gpu
def test_an_lp_does_not_see_its_neighbours_and_a_batch_of_one_is_the_unbatched_loop():
    full = loop_run(BatchedDeviceHSD, "K1", "failed")
    lps = bump_copies(6)
    # other neighbours, another slot: LPs 4, 1 and a well-behaved LP in between
    opt = BatchedDeviceHSD([lps[4], golden("lpex_opt"), lps[1]], device=0, options=Forty(), retry="failed").optimize()
    same_record(record_of(opt, 0), full["recs"][4], "LP 4 with other neighbours")
    same_record(record_of(opt, 2), full["recs"][1], "LP 1 with other neighbours")
    opt.kkt.close()
    # B = 1 against DeviceHSD
    d = lps[0]
    one = DeviceHSD(d[0], d[1], d[2], d[3], d[4], c0=d[5], objsense_min=d[6], device=0, options=Forty()).optimize()
    b1 = BatchedDeviceHSD([d], device=0, options=Forty(), retry="failed").optimize()
    assert one.timers["n_bump"] > 0, "bad test input: the copy never bumps"
    assert b1.status[0] == one.status and b1.niter[0] == one.niter and b1.timers_of(0)["n_bump"] == one.timers["n_bump"]
    assert b1.timers_of(0)["n_update"] == one.timers["n_update"]
    for code, length in ((0, one.n), (1, one.n), (2, one.n), (3, one.n), (4, one.n), (5, one.m)):
        assert bits(b1._get(0, code), one._get(code, length)), code
    same_record(record_of(b1, 0), full["recs"][0], "LP 0 alone")
    one.kkt.close(); b1.kkt.close()


@pytest.mark.gpu
def test_a_refused_hold_falls_back_to_whole_updates_with_one_warning():
    """refine = 1: the library refuses the hold, the loop goes on with whole updates and ends as retry='all' does."""
    lps = bump_copies(3)
    ref = BatchedDeviceHSD(lps, device=0, options=Forty(), refine=1, retry="all").optimize()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        opt = BatchedDeviceHSD(lps, device=0, options=Forty(), refine=1, retry="failed").optimize()
    told = [w for w in caught if "falling back to retry='all'" in str(w.message)]
    assert ref.timers["n_bump"].sum() > 0, "bad test input"
    assert len(told) == 1 and opt.retry == "all"
    for k in range(3):
        same_record(record_of(opt, k), record_of(ref, k), f"LP {k}")
    ref.kkt.close(); opt.kkt.close()
