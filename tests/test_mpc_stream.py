"""The Mehrotra batch as a stream (`tlpk_mpc_batch_factor_enter`, `tlpk_mpc_batch_newton_enter`, `tlpk_mpc_batch_enter_finish`, `tlpk_ipm_get_lps`,
`BatchedDeviceMPC.refill` / `optimize_stream`, `Model.optimize_stream`): an LP that takes a slot ENTERS through the update and the two solves of the
running LPs.  CPU: the ABI surface, the refusals in their order, the refusals of the Python layer.  GPU (K1, K2; skip_parked off and on): with no
entering LP each call is its counterpart bit for bit; with every LP entering the four calls are tlpk_mpc_batch_start; an entering LP and its
neighbours do not see each other, a parked LP keeps every bit; the gather of the records equals the per-LP reads; an LP that streams through a slot
is the LP of one plain batch, bit for bit; two patterns in one handle; an entering LP that fails its update; the Model front door.

Shapes: the three LPs of test_hsd_stream.boundary_slots (1 x 1, 9 x 257, 8 x 256: the segment edges of the 256-thread block tables) and its `family`
(12 x 30, one pattern)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tulip_jl_amd as tk
from test_hsd_batch import EXAMPLES, GOLDEN, ROOT, load_batch, small_lps, stacked_handle
from test_hsd_stream import bits, boundary_slots, family, get_all
from tulip_jl_amd import _lib
from tulip_jl_amd.hsd_batch import BatchedDeviceHSD
from tulip_jl_amd.hsd_device import Options
from tulip_jl_amd.mpc_batch import BatchedDeviceMPC

ENTER_SYMBOLS = ["tlpk_mpc_batch_factor_enter", "tlpk_mpc_batch_newton_enter", "tlpk_mpc_batch_enter_finish", "tlpk_ipm_get_lps"]
pu8, pd, p64 = _lib.as_pu8, _lib.as_pd, _lib.as_p64
p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))                      # noqa: E731


def u8(*flags):
    return np.array(flags, dtype=np.uint8)


def last_error(h):
    return _lib.lib().tlpk_last_error(h).decode()


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_enter_symbols_are_declared_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "tlpk.h")).read()
    L = _lib.lib()
    for name in ENTER_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
        assert getattr(L, name).restype is C.c_int and getattr(L, name).argtypes, name
    for name in ENTER_SYMBOLS:                                              # tests/test_api_contract.py tabulates these families by prefix
        assert not name.startswith(("tlpk_update", "tlpk_solve", "tlpk_refine", "tlpk_root", "tlpk_sync")), name


def test_the_enter_calls_refuse_in_order_without_a_load():
    A, ro, co, vecs = stacked_handle()
    L = _lib.lib()
    act, ent, clash = u8(1, 0, 0), u8(0, 1, 0), u8(1, 1, 0)
    d = np.ones(16); fail = C.c_int64(7)
    what, lps, x = np.array([0, 5], dtype=np.int32), np.array([1, 0], dtype=np.int64), np.zeros(64)
    # a NULL handle
    assert L.tlpk_mpc_batch_factor_enter(None, pu8(act), pu8(ent), pd(d), pd(d), C.byref(fail)) == _lib.BADARG
    assert L.tlpk_mpc_batch_newton_enter(None, 0, pu8(act), pu8(ent), pd(d), pd(d)) == _lib.BADARG
    assert L.tlpk_mpc_batch_enter_finish(None, pu8(ent), pd(d)) == _lib.BADARG
    assert L.tlpk_ipm_get_lps(None, p32(what), 2, p64(lps), 2, pd(x), 24) == _lib.BADARG
    # an analyse-only handle, on which nothing can be loaded: "load first" comes before the NULL pointers, the role clash, the mode and the missing device
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=-1, row_block=np.repeat(np.arange(3), np.diff(ro))))
    assert load_batch(kkt, 3, ro, co, vecs)[0] == _lib.NO_DEVICE
    calls = [lambda a=act, e=ent, out=d: L.tlpk_mpc_batch_factor_enter(kkt._h, pu8(a), None if e is None else pu8(e), pd(d), pd(d), None if out is None else C.byref(fail)),
             lambda a=act, e=ent, out=d, mode=0: L.tlpk_mpc_batch_newton_enter(kkt._h, mode, pu8(a), None if e is None else pu8(e), pd(d), None if out is None else pd(out)),
             lambda a=act, e=ent, out=d: L.tlpk_mpc_batch_enter_finish(kkt._h, None if e is None else pu8(e), None if out is None else pd(out))]
    for call in calls:
        for kw in ({}, {"e": None}, {"out": None}, {"a": clash, "e": clash}):
            assert call(**kw) == _lib.BADARG and "load first" in last_error(kkt._h), kw
    assert calls[1](mode=2) == _lib.BADARG and "load first" in last_error(kkt._h)
    # tlpk_ipm_get_lps refuses as tlpk_ipm_get_lp does on this handle
    assert L.tlpk_ipm_get_lps(kkt._h, p32(what), 2, p64(lps), 2, pd(x), 24) == L.tlpk_ipm_get_lp(kkt._h, 0, 1, pd(x), 9)
    kkt.close()


def test_python_refusals_need_no_gpu():
    fam = family(4)
    opt = BatchedDeviceMPC(fam[:2], device=-1, load=False)
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
    with pytest.raises(ValueError, match="one LP per listed slot"):
        opt.refill([0, 0], [fam[2], fam[3]])
    for a, b in zip(before, (opt.A.data, opt._b, opt._c, opt._l, opt._u)):
        assert bits(a, b)                                                # nothing was changed
    opt.kkt.close()


def test_model_optimize_stream_checks_its_arguments():
    paths = [os.path.join(GOLDEN, name + ".mps") for name in EXAMPLES[:2]]
    load = lambda **kw: [tk.Model.load(p, **kw) for p in paths]             # noqa: E731
    with pytest.raises(ValueError, match="slots must be at least 1"):
        tk.Model.optimize_stream(load(algorithm="mpc"), 0, device=-1)
    with pytest.raises(TypeError, match="integer"):
        tk.Model.optimize_stream(load(algorithm="mpc"), 2.5, device=-1)
    with pytest.raises(TypeError, match="integer"):
        tk.Model.optimize_stream(load(algorithm="mpc"), True, device=-1)
    with pytest.raises(TypeError, match="Model"):
        tk.Model.optimize_stream(load() + ["lpex_opt.mps"], 2, device=-1)
    with pytest.raises(ValueError, match="algorithm"):
        tk.Model.optimize_stream(load(algorithm="simplex"), 2, device=-1)
    assert tk.Model.optimize_stream([], 2, device=-1) == []
    with pytest.raises(ValueError, match=r"mpc.*Model\.optimize_stream"):      # the pinned refusal now says where to go
        tk.Model.optimize_batch(load(algorithm="mpc"), slots=2, device=-1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the calls
# ---------------------------------------------------------------------------------------------------------------------------------------
CASES = [("K1", False), ("K1", True), ("K2", False), ("K2", True)]
CASE_IDS = ["K1", "K1-skip", "K2", "K2-skip"]
ALL = range(36)


def four_lps():
    """The three boundary shapes and one LP of the family."""
    return boundary_slots(1) + [family(2)[1]]


def loaded(lps, sysname, skip):
    A, ro, co, vecs = stacked_handle(lps)
    kkt = tk.setup(A, tk.K1() if sysname == "K1" else tk.K2(), tk.Backend(device=0, row_block=np.repeat(np.arange(len(lps)), np.diff(ro))))
    assert load_batch(kkt, len(lps), ro, co, vecs)[0] == _lib.OK
    if skip:
        assert _lib.lib().tlpk_ipm_batch_skip(kkt._h, 1) == _lib.OK
    return kkt


def same_vectors(a, b, codes, label):
    va, vb = get_all(a, codes), get_all(b, codes)
    for what in codes:
        assert bits(va[what], vb[what]), (label, what, np.flatnonzero(va[what] != vb[what])[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("sysname,skip", CASES, ids=CASE_IDS)
def test_without_entering_lps_each_call_is_its_counterpart(sysname, skip):
    """Contract (a), on twin handles: one LP of the four is parked, so the parking and the mask are part of what is compared."""
    L = _lib.lib()
    lps = four_lps()
    B = len(lps)
    one, two = loaded(lps, sysname, skip), loaded(lps, sysname, skip)
    act, none = u8(1, 1, 0, 1), np.zeros(B, dtype=np.uint8)
    o1, o2 = np.zeros(B), np.zeros(B)
    assert L.tlpk_mpc_batch_start(one._h, pd(o1)) == _lib.OK and L.tlpk_mpc_batch_start(two._h, pd(o2)) == _lib.OK and bits(o1, o2)
    res = np.zeros(13 * B)
    for kkt in (one, two):
        assert L.tlpk_ipm_batch_residuals(kkt._h, pd(np.ones(B)), pd(res)) == _lib.OK
    regP, regD = np.full(B, 0.1), np.full(B, 0.01)
    f1, f2 = C.c_int64(7), C.c_int64(7)
    assert L.tlpk_ipm_batch_factor(one._h, pu8(act), pd(regP), pd(regD), C.byref(f1)) == _lib.OK
    assert L.tlpk_mpc_batch_factor_enter(two._h, pu8(act), pu8(none), pd(regP), pd(regD), C.byref(f2)) == _lib.OK
    assert f1.value == f2.value == -1
    same_vectors(one, two, ALL, "factor")
    gmu = np.zeros(B)
    for mode in (0, 1):
        s1, s2 = np.full((B, 2), 7.0), np.full((B, 2), 7.0)
        assert L.tlpk_mpc_batch_newton(one._h, mode, pu8(act), pd(gmu), pd(s1)) == _lib.OK
        assert L.tlpk_mpc_batch_newton_enter(two._h, mode, pu8(act), pu8(none), pd(gmu), pd(s2)) == _lib.OK
        assert bits(s1, s2) and not s2[2].any() and (s2[[0, 1, 3]] > 0).all(), (mode, s1, s2)
        same_vectors(one, two, ALL, f"newton {mode}")
        g1, g2 = np.zeros((B, 2)), np.zeros((B, 2))
        ap, ad = np.minimum(1.0, s1[:, 0]).copy(), np.minimum(1.0, s1[:, 1]).copy()
        for kkt, g in ((one, g1), (two, g2)):
            assert L.tlpk_mpc_batch_gap(kkt._h, pu8(act), pd(ap), pd(ad), pd(g)) == _lib.OK
        assert bits(g1, g2)
        gmu = np.ascontiguousarray(0.1 * g1[:, 1] / 7.0)                      # some centring for the corrector
    before = get_all(two, ALL)
    out = np.full(B, 7.0)
    assert L.tlpk_mpc_batch_enter_finish(two._h, pu8(none), pd(out)) == _lib.OK and not out.any()      # its counterpart with nothing entering: nothing
    after = get_all(two, ALL)
    for what in ALL:
        assert bits(before[what], after[what]), ("finish", what)
    one.close(); two.close()


def enter_sequence(kkt, act, ent, regP=None, regD=None):
    """factor_enter, newton_enter(0), newton_enter(1), enter_finish with the given roles; returns enter_finish's out."""
    L = _lib.lib()
    B = act.shape[0]
    fail = C.c_int64(7)
    regP = np.ones(B) if regP is None else regP
    regD = np.ones(B) if regD is None else regD
    assert L.tlpk_mpc_batch_factor_enter(kkt._h, pu8(act), pu8(ent), pd(regP), pd(regD), C.byref(fail)) == _lib.OK and fail.value == -1
    for mode in (0, 1):
        s = np.full((B, 2), 7.0)
        assert L.tlpk_mpc_batch_newton_enter(kkt._h, mode, pu8(act), pu8(ent), pd(np.zeros(B)), pd(s)) == _lib.OK
        assert not s[ent != 0].any()                                         # an entering LP's out is 0
    out = np.full(B, 7.0)
    assert L.tlpk_mpc_batch_enter_finish(kkt._h, pu8(ent), pd(out)) == _lib.OK
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("sysname,skip", CASES, ids=CASE_IDS)
def test_with_every_lp_entering_the_four_calls_are_the_starting_point(sysname, skip):
    """Contract (b)."""
    L = _lib.lib()
    lps = four_lps()
    B = len(lps)
    ref, kkt = loaded(lps, sysname, skip), loaded(lps, sysname, skip)
    o_ref = np.zeros(B)
    assert L.tlpk_mpc_batch_start(ref._h, pd(o_ref)) == _lib.OK
    out = enter_sequence(kkt, np.zeros(B, dtype=np.uint8), np.ones(B, dtype=np.uint8))
    print("xl'zl + xu'zu of the starting points", o_ref)
    assert bits(out, o_ref) and (o_ref > 0).all()
    same_vectors(ref, kkt, ALL, "start")                                     # (0 - 32 are the contract; 33 - 35 are the starting matrix both wrote)
    x = get_all(kkt, [0, 5])
    assert x[0].any() and x[5].any()
    ref.close(); kkt.close()


def mpc_pass(opt, act, enter=None):
    opt.compute_residuals(act); opt.update_solver_status(act)
    if enter is None:
        return opt.compute_step(act)
    return opt._step_stream(act, enter)


def segments(opt, k, codes=range(33)):
    return {what: opt._get_lp(k, what) for what in codes}


STARTING_POINT_WRITES = (0, 1, 2, 3, 4, 5, 6, 11, 24, 25, 31, 32)           # the iterate, the two halves kept in the accepted direction (x, y), hx, hy, xid, xip


@pytest.mark.gpu
@pytest.mark.parametrize("sysname,skip", CASES, ids=CASE_IDS)
def test_an_entering_lp_and_its_neighbours_do_not_see_each_other(sysname, skip):
    """Contracts (c) and (d).  Two passes of the plain batch on (a, b, c); on a twin, slot 1 is refilled with d after pass 1 and d enters during pass 2.
    After enter_finish slot 1 is compared with a fresh handle on (a, d, c) after tlpk_mpc_batch_start in every vector the starting point writes
    (STARTING_POINT_WRITES; the residuals, theta halves and the other right-hand sides of the slot are its former LP's, as after any refill)."""
    a, b, c = boundary_slots(1)
    d = boundary_slots(2)[1]
    kw = dict(system=sysname, device=0, skip_parked=skip)
    T, F = True, False
    every = np.array([T, T, T])
    with np.errstate(all="ignore"):
        plain = BatchedDeviceMPC([a, b, c], **kw); plain._init_state(); plain.compute_starting_point()
        assert mpc_pass(plain, every).all() and mpc_pass(plain, every).all()
        twin = BatchedDeviceMPC([a, b, c], **kw); twin._init_state(); twin.compute_starting_point()
        assert mpc_pass(twin, every).all()
        BatchedDeviceHSD.refill(twin, [1], [d])                              # tlpk_ipm_batch_refill alone: the starting point is to ride in pass 2
        moved, entered = mpc_pass(twin, np.array([T, F, T]), np.array([F, T, F]))
        assert moved.tolist() == [T, F, T] and entered.tolist() == [F, T, F]
        fresh = BatchedDeviceMPC([a, d, c], **kw); fresh._init_state(); fresh.compute_starting_point()
        # (d) a parked LP: a third handle repeats the twin's pass 2 with slot 2 neither active nor entering
        park = BatchedDeviceMPC([a, b, c], **kw); park._init_state(); park.compute_starting_point()
        assert mpc_pass(park, every).all()
        BatchedDeviceHSD.refill(park, [1], [d])
        park.compute_residuals(np.array([T, F, F]))                          # (the residual call has no mask: it rewrites the residuals of every LP from its iterate)
        kept = segments(park, 2)
        moved, entered = park._step_stream(np.array([T, F, F]), np.array([F, T, F]))
        assert moved.tolist() == [T, F, F] and entered.tolist() == [F, T, F]
    for k in (0, 2):
        va, vb = segments(plain, k), segments(twin, k)
        for what in va:
            assert bits(va[what], vb[what]), ("neighbour", k, what)
    for name in ("mu", "alpha_p", "alpha_d", "regP", "regD"):
        assert bits(getattr(plain, name)[[0, 2]], getattr(twin, name)[[0, 2]]), name
    va, vb, vp = segments(fresh, 1, STARTING_POINT_WRITES), segments(twin, 1, STARTING_POINT_WRITES), segments(park, 1, STARTING_POINT_WRITES)
    for what in STARTING_POINT_WRITES:
        assert bits(va[what], vb[what]), ("entered", what, np.abs(va[what] - vb[what]).max())
        assert bits(va[what], vp[what]), ("entered beside a parked LP", what)
    assert va[0].any() and va[5].any() and bits(fresh.mu[1], twin.mu[1]) and bits(fresh.mu[1], park.mu[1])
    assert twin.timers_of(1)["n_update"] == 1 and twin.timers_of(1)["n_solve"] == 2      # as compute_starting_point counts them
    after = segments(park, 2)
    for what in kept:
        assert bits(kept[what], after[what]), ("parked", what)
    va, vb = segments(plain, 0), segments(park, 0)
    for what in va:
        assert bits(va[what], vb[what]), ("beside a parked LP", what)
    for opt in (plain, twin, fresh, park):
        opt.kkt.close()


@pytest.mark.gpu
def test_a_role_clash_and_mode_2_are_refused():
    L = _lib.lib()
    lps = boundary_slots(1)
    kkt = loaded(lps, "K1", False)
    d = np.ones(3); out = np.zeros(6); fail = C.c_int64(7)
    start = np.zeros(3)
    assert L.tlpk_mpc_batch_start(kkt._h, pd(start)) == _lib.OK
    before = get_all(kkt, ALL)
    act, ent, clash = u8(1, 0, 1), u8(0, 1, 0), u8(0, 1, 1)
    assert L.tlpk_mpc_batch_factor_enter(kkt._h, pu8(act), pu8(clash), pd(d), pd(d), C.byref(fail)) == _lib.BADARG
    assert "LP 2 is both active and entering" in last_error(kkt._h)
    assert L.tlpk_mpc_batch_newton_enter(kkt._h, 0, pu8(act), pu8(clash), pd(d), pd(out)) == _lib.BADARG
    assert "both active and entering" in last_error(kkt._h)
    assert L.tlpk_mpc_batch_newton_enter(kkt._h, 2, pu8(act), pu8(ent), pd(d), pd(out)) == _lib.BADARG and "mode" in last_error(kkt._h)
    assert L.tlpk_mpc_batch_newton_enter(kkt._h, -1, pu8(act), pu8(ent), pd(d), pd(out)) == _lib.BADARG
    # NULL pointers come before the clash
    assert L.tlpk_mpc_batch_factor_enter(kkt._h, pu8(clash), pu8(clash), pd(d), pd(d), None) == _lib.BADARG and "NULL" in last_error(kkt._h)
    assert L.tlpk_mpc_batch_newton_enter(kkt._h, 0, pu8(clash), pu8(clash), None, pd(out)) == _lib.BADARG and "NULL" in last_error(kkt._h)
    assert L.tlpk_mpc_batch_enter_finish(kkt._h, None, pd(out)) == _lib.BADARG and "NULL" in last_error(kkt._h)
    after = get_all(kkt, ALL)
    for what in ALL:
        assert bits(before[what], after[what]), what                         # a refused call writes nothing
    # the stale handle comes before the clash
    nz = stacked_handle(lps)[0].data.copy()
    assert L.tlpk_set_values(kkt._h, pd(nz), nz.shape[0]) == _lib.OK
    assert L.tlpk_mpc_batch_factor_enter(kkt._h, pu8(clash), pu8(clash), pd(d), pd(d), C.byref(fail)) == _lib.BADARG and "tlpk_ipm_reload" in last_error(kkt._h)
    assert L.tlpk_mpc_batch_enter_finish(kkt._h, pu8(ent), pd(out)) == _lib.BADARG and "tlpk_ipm_reload" in last_error(kkt._h)
    kkt.close()
    # a handle that holds one LP (tlpk_ipm_load) is not batch-loaded: refused before the NULL pointers
    A, b, c, l, u = lps[1]
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=0))
    assert L.tlpk_ipm_load(kkt._h, pd(b), pd(c), pd(l), pd(u)) == _lib.OK
    assert L.tlpk_mpc_batch_factor_enter(kkt._h, pu8(act), None, pd(d), pd(d), C.byref(fail)) == _lib.BADARG and "tlpk_ipm_load_batch" in last_error(kkt._h)
    assert L.tlpk_mpc_batch_newton_enter(kkt._h, 2, pu8(act), pu8(ent), pd(d), None) == _lib.BADARG and "tlpk_ipm_load_batch" in last_error(kkt._h)
    assert L.tlpk_mpc_batch_enter_finish(kkt._h, None, pd(out)) == _lib.BADARG and "tlpk_ipm_load_batch" in last_error(kkt._h)
    kkt.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sysname", ["K1", "K2"])
def test_get_lps_equals_the_per_lp_reads(sysname):
    L = _lib.lib()
    lps = four_lps()
    kkt = loaded(lps, sysname, False)
    _, ro, co, _ = stacked_handle(lps)
    out = np.zeros(4)
    assert L.tlpk_mpc_batch_start(kkt._h, pd(out)) == _lib.OK
    res = np.zeros(13 * 4)
    assert L.tlpk_ipm_batch_residuals(kkt._h, pd(np.ones(4)), pd(res)) == _lib.OK

    def length(k, what):
        off = ro if what in _lib.IPM_GET_ROWS else co
        return int(off[k + 1] - off[k])

    def one_by_one(codes, ks):
        parts = []
        for k in ks:
            for what in codes:
                v = np.empty(length(k, what))
                assert L.tlpk_ipm_get_lp(kkt._h, what, k, pd(v), v.shape[0]) == _lib.OK
                parts.append(v)
        return np.concatenate(parts) if parts else np.zeros(0)

    def gathered(codes, ks, pad=0):
        what, lp = np.array(codes, dtype=np.int32), np.array(ks, dtype=np.int64)
        buf = np.full(sum(length(k, w) for k in ks for w in codes) + pad, 7.0)
        return L.tlpk_ipm_get_lps(kkt._h, p32(what), len(codes), p64(lp), len(ks), pd(buf), buf.shape[0] - pad), buf

    for codes, ks in (([5, 0, 18, 3, 32, 35, 21], [2, 0, 3, 1]), ([0], [1]), ([25, 5], [0]), (list(range(36)), [3, 2, 1, 0]), ([4, 4], [1, 2])):
        rc, buf = gathered(codes, ks, pad=3)
        ref = one_by_one(codes, ks)
        assert rc == _lib.OK and ref.any()
        assert bits(buf[:-3], ref) and (buf[-3:] == 7.0).all(), (codes, ks)
    # refusals: a wrong len, a repeated LP, an LP out of range, a code out of range, NULL
    what, lp, buf = np.array([0, 5], dtype=np.int32), np.array([1, 2], dtype=np.int64), np.zeros(600)
    need = length(1, 0) + length(1, 5) + length(2, 0) + length(2, 5)
    assert L.tlpk_ipm_get_lps(kkt._h, p32(what), 2, p64(lp), 2, pd(buf), need) == _lib.OK
    assert L.tlpk_ipm_get_lps(kkt._h, p32(what), 2, p64(lp), 2, pd(buf), need + 1) == _lib.BADARG and "length" in last_error(kkt._h)
    for bad, word in (([1, 1], "twice"), ([1, 4], "LP 4"), ([-1, 1], "LP -1")):
        lp = np.array(bad, dtype=np.int64)
        assert L.tlpk_ipm_get_lps(kkt._h, p32(what), 2, p64(lp), 2, pd(buf), need) == _lib.BADARG and word in last_error(kkt._h), bad
    lp = np.array([1, 2], dtype=np.int64)
    assert L.tlpk_ipm_get_lps(kkt._h, p32(np.array([0, 36], dtype=np.int32)), 2, p64(lp), 2, pd(buf), need) == _lib.BADARG
    assert L.tlpk_ipm_get_lps(kkt._h, None, 2, p64(lp), 2, pd(buf), need) == _lib.BADARG
    assert L.tlpk_ipm_get_lps(kkt._h, p32(what), 2, p64(lp), 2, None, need) == _lib.BADARG
    kkt.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the stream
# ---------------------------------------------------------------------------------------------------------------------------------------
_plain = {}
COMPARED = ("x", "y", "zl", "zu")


def plain_run(name, lps, system, options=None):
    """One plain BatchedDeviceMPC(lps).optimize(), computed once per (name, system) and shared: what every LP of a stream is held to."""
    if (name, system) not in _plain:
        opt = BatchedDeviceMPC(lps, system=system, device=0, options=options).optimize()
        out = []
        for k in range(len(lps)):
            out.append(dict(opt.solution(k), zl=opt._get(k, 3), zu=opt._get(k, 4), timers=opt.timers_of(k),
                            primal_objective=float(opt.primal_objective[k]), dual_objective=float(opt.dual_objective[k])))
        opt.kkt.close()
        _plain[(name, system)] = out
    return _plain[(name, system)]


def assert_same_run(rec, ref, label):
    print(f"  {label}: slot {rec['slot']} passes {rec['entered']}..{rec['left']}  {rec['status']:22s} niter {rec['niter']:3d} / {ref['niter']:3d}  "
          f"z {rec['z_primal']:.12e} / {ref['z_primal']:.12e}")
    assert rec["status"] == ref["status"] and rec["niter"] == ref["niter"], label
    assert rec["primal_status"] == ref["primal_status"] and rec["dual_status"] == ref["dual_status"], label
    for key in COMPARED:
        assert bits(rec[key], ref[key]), (label, key, np.abs(rec[key] - ref[key]).max())
    for key in ("z_primal", "z_dual", "primal_objective", "dual_objective"):
        assert bits(rec[key], ref[key]), (label, key, rec[key], ref[key])
    assert rec["timers"] == ref["timers"], (label, rec["timers"], ref["timers"])


@pytest.mark.gpu
@pytest.mark.parametrize("sysname,skip", CASES, ids=CASE_IDS)
def test_streaming_equals_one_plain_batch(sysname, skip):
    fam = family(7)
    opt = BatchedDeviceMPC(fam[:3], system=sysname, device=0, skip_parked=skip)
    records = opt.optimize_stream(fam[3:])
    ref = plain_run("family7", fam, sysname)
    print(sysname, "skip_parked", skip, "passes", opt.passes, "refills", opt.refills)
    assert len(records) == 7 and [r["slot"] for r in records[:3]] == [0, 1, 2] and all(r["entered"] == 1 for r in records[:3])
    for i, (rec, r) in enumerate(zip(records, ref)):
        assert_same_run(rec, r, f"LP {i}")
    # the test cannot pass on a degenerate run
    assert sum(r["status"] == "Trm_Optimal" for r in records) >= 5, [r["status"] for r in records]
    assert len({r["niter"] for r in records}) >= 3, [r["niter"] for r in records]
    # the schedule: a slot holds an LP for niter + 1 passes, its successor enters in the pass in which it leaves
    for r in records:
        assert r["left"] - r["entered"] == r["niter"], r
    for r in records[3:]:
        assert any(p["slot"] == r["slot"] and p["left"] + 1 == r["entered"] for p in records), r
    assert opt.passes == max(r["left"] for r in records) and opt.refills >= 2
    opt.kkt.close()


@pytest.mark.gpu
def test_options_travel_with_the_lp():
    class TwentyIterations(Options):
        IterationsLimit = 20

    fam = family(8)
    opt = BatchedDeviceMPC(fam[:2], device=0)
    records = opt.optimize_stream([fam[7], fam[2]], options=[TwentyIterations(), Options()])
    assert records[2]["status"] == "Trm_IterationLimit" and records[2]["niter"] == 20 and records[2]["left"] - records[2]["entered"] == 20
    alone = plain_run("family8[7]", [fam[7]], "K1", options=[TwentyIterations()])
    assert_same_run(records[2], alone[0], "the eighth LP")
    ref = plain_run("family7", family(7), "K1")
    for i in (0, 1):
        assert_same_run(records[i], ref[i], f"LP {i}")
    assert_same_run(records[3], ref[2], "LP 2")
    k = records[3]["slot"]                                                   # whichever slot LP 2 took runs under LP 2's options
    assert opt.opts[k].IterationsLimit == Options().IterationsLimit and opt._o["IterationsLimit"][k] == Options().IterationsLimit
    opt.kkt.close()


@pytest.mark.gpu
@pytest.mark.parametrize("skip", [False, True], ids=["all-blocks", "skip"])
def test_two_patterns_in_one_handle(skip):
    fam = family(7)
    b1, b2, b3 = boundary_slots(1), boundary_slots(2), boundary_slots(3)
    first = [fam[0], b1[0], b1[1], b1[2]]                                    # slot 0: the family's pattern; slots 1 - 3: 1 x 1, 9 x 257, 8 x 256
    queue = [fam[1], b2[1], fam[2], b2[0], fam[3], b2[2], b3[1], fam[4], fam[5], fam[6]]
    slot_of = [0, 1, 2, 3] + [0, 2, 0, 1, 0, 3, 2, 0, 0, 0]
    opt = BatchedDeviceMPC(first, device=0, skip_parked=skip)
    records = opt.optimize_stream(queue)
    assert [r["slot"] for r in records] == slot_of                           # every LP ran in a slot of its own pattern
    ref = plain_run("two patterns", first + queue, "K1")
    for i, (rec, r) in enumerate(zip(records, ref)):
        assert_same_run(rec, r, f"LP {i}")
    for k in range(4):                                                       # FIFO per pattern: the LPs of a slot ran in queue order, one after the other
        mine = [r for r in records if r["slot"] == k]
        assert all(q["entered"] == p["left"] + 1 for p, q in zip(mine, mine[1:])), k
    assert len({r["niter"] for r in records}) >= 3, "bad test input: the LPs should differ in length"
    opt.kkt.close()


@pytest.mark.gpu
@pytest.mark.parametrize("skip", [False, True], ids=["all-blocks", "skip"])
def test_an_entering_lp_that_fails_its_update_frees_its_slot(skip):
    """The LP that fails: one entry of A is not a number, so the pivot of its row of A A' + 1e-6 I is refused whatever the regularisation (the starting
    point's are constants: there is nothing to bump)."""
    fam = family(7)
    A = fam[3][0].copy(); A.data[0] = np.nan
    bad = (A,) + tuple(fam[3][1:])
    opt = BatchedDeviceMPC(fam[:3], device=0, skip_parked=skip)
    records = opt.optimize_stream([fam[3], bad, fam[4], fam[5], fam[6]])
    rec = records[4]
    assert rec["status"] == "Trm_NumericalProblem" and rec["niter"] == 0 and rec["entered"] == rec["left"]
    assert rec["timers"]["n_update"] == 0 and rec["timers"]["n_bump"] == 0
    after = [r for r in records if r["slot"] == rec["slot"] and r["entered"] > rec["left"]]
    assert after and min(r["entered"] for r in after) == rec["left"] + 2     # the slot is refilled in the next pass: its LP enters there and is active in the one after
    ref = plain_run("family7", fam, "K1")
    others = records[:4] + records[5:]
    for i, (r, p) in enumerate(zip(others, ref)):
        assert_same_run(r, p, f"LP {i}")                                      # bit-identical to the run without the failing LP
    opt.kkt.close()


@pytest.mark.gpu
def test_refill_runs_the_starting_point_for_its_slots_alone():
    a, b, c = boundary_slots(1)
    d = boundary_slots(2)[1]
    with np.errstate(all="ignore"):
        opt = BatchedDeviceMPC([a, b, c], device=0); opt._init_state(); opt.compute_starting_point()
        every = np.array([True] * 3)
        assert mpc_pass(opt, every).all()
        kept = {k: segments(opt, k) for k in (0, 2)}
        opt.refill([1], [d])
        fresh = BatchedDeviceMPC([a, d, c], device=0); fresh._init_state(); fresh.compute_starting_point()
    for k in (0, 2):
        now = segments(opt, k)
        for what in now:
            assert bits(kept[k][what], now[what]), (k, what)
    va, vb = segments(fresh, 1, STARTING_POINT_WRITES), segments(opt, 1, STARTING_POINT_WRITES)
    for what in STARTING_POINT_WRITES:
        assert bits(va[what], vb[what]), what
    assert bits(fresh.mu[1], opt.mu[1]) and opt.niter[1] == 0 and opt.status[1] == "Trm_Unknown" and opt.regP[1] == 1.0 and opt.kappa[1] == 0.0
    opt.kkt.close(); fresh.kkt.close()


@pytest.mark.gpu
def test_model_optimize_stream():
    paths = [os.path.join(GOLDEN, name + ".mps") for name in EXAMPLES] + [os.path.join(GOLDEN, "lpex_opt.mps")] * 2

    def load(**kw):
        models = [tk.Model.load(p, algorithm="mpc", **kw) for p in paths]
        for mdl, f in zip(models[4:], (1.03, 0.96)):
            mdl.lp.obj = mdl.lp.obj * f
        return models

    own = [m.optimize() for m in load(device=0)]
    models = tk.Model.optimize_stream(load(), 2, device=0)
    print([(m.status, m.inner is None) for m in own])
    for a, b in zip(models, own):
        assert a.status == b.status
        assert (a.inner is None) == (b.inner is None)            # (a model presolve alone solves never reaches the stream)
        for f in ("objective_value", "dual_objective_value"):
            za, zb = getattr(a, f)(), getattr(b, f)()
            assert (za == zb) or abs(za - zb) <= 1e-9 * (1 + abs(zb)), (f, za, zb)
    assert [m.status for m in own[4:]] == ["Trm_Optimal"] * 2 and own[0].status == "Trm_Optimal"
    assert sum(m.inner is not None for m in models) >= 3, "bad test input: the stream needs more LPs than slots"
    # mixed algorithms stream side by side, each through its own loop
    mixed = load()
    for mdl in mixed[::2]:
        mdl.algorithm = "hsd"
    mixed = tk.Model.optimize_stream(mixed, 2, skip_parked=True, device=0)
    assert [m.status for m in mixed] == [m.status for m in own]
