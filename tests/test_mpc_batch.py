"""Batched device-resident MPC (`tlpk_mpc_batch_*`, `BatchedDeviceMPC`, `Model.optimize_batch` with algorithm="mpc"): Mehrotra's loop on a
stack of LPs with per-LP scalars and masks.  CPU: the ABI surface, the refusals, the stacking, and the host loop's mask logic on the float64
stand-in of tests/ipm_reference.py (the five batched calls built from its unbatched ones: the batch must reproduce `DeviceMPC` LP by LP).
The per-call checks are written once and run on the stand-in (any machine) and on libtlpk.so (`-m gpu`): every call against long double per
segment (|device - r| <= 2 K u M, tests/ipm_reference.py), an inactive LP is not written and returns 0, a one-LP batch is the unbatched
call bit for bit.  GPU only: the loop held to `DeviceMPC`'s own record of each LP with the tolerances of tests/test_hsd_batch.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ipm_reference as ir
import tulip_jl_amd as tk
from ipm_harness import read_free_mps, standard_form
from test_hsd_batch import (EXAMPLE_STATUS, EXAMPLES, GOLDEN, ROOT, SQRT_EPS, boundary_lps, close_to, golden, load_batch, of_batch, small_lps,
                            stacked_handle)
from test_ipm_kernels import DRIVERS, MPC_SC, SHAPES, Driver, Table, _Holder, _standin_loop, lp_of, pd
from tulip_jl_amd import _lib
from tulip_jl_amd.hsd_device import Options
from tulip_jl_amd.mpc_batch import BatchedDeviceMPC
from tulip_jl_amd.mpc_device import DeviceMPC

MPC_BATCH_SYMBOLS = ["tlpk_mpc_batch_start", "tlpk_mpc_batch_newton", "tlpk_mpc_batch_gap", "tlpk_mpc_batch_targets", "tlpk_mpc_batch_advance"]
pu8 = _lib.as_pu8


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: the surface
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_mpc_batch_symbols_are_declared_exported_and_listed():
    header = open(os.path.join(ROOT, "include", "tlpk.h")).read()
    L = _lib.lib()
    for name in MPC_BATCH_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
        assert getattr(L, name).restype is C.c_int and getattr(L, name).argtypes, name


def mpc_batch_calls(L, h, nlp=3):
    act = np.ones(nlp, dtype=np.uint8); d = np.ones(16 * nlp)
    return {"start": lambda out=d: L.tlpk_mpc_batch_start(h, None if out is None else pd(out)),
            "newton": lambda mode=0, a=act, g=d, out=d: L.tlpk_mpc_batch_newton(h, mode, *[None if v is None else (pu8(v) if v is act else pd(v)) for v in (a, g, out)]),
            "gap": lambda a=act, p=d, q=d, out=d: L.tlpk_mpc_batch_gap(h, *[None if v is None else (pu8(v) if v is act else pd(v)) for v in (a, p, q, out)]),
            "targets": lambda a=act, par=d: L.tlpk_mpc_batch_targets(h, None if a is None else pu8(a), None if par is None else pd(par)),
            "advance": lambda a=act, p=d, q=d, out=d: L.tlpk_mpc_batch_advance(h, *[None if v is None else (pu8(v) if v is act else pd(v)) for v in (a, p, q, out)])}


def test_the_calls_refuse_what_they_cannot_serve():
    """Without a device nothing can be loaded: tlpk_ipm_load_batch answers TLPK_NO_DEVICE on the analyse-only handle and the five calls the
    load-order sentence (the order of the existing batched calls: the load is checked before the device).  NULL handle, NULL pointers: BADARG."""
    A, ro, co, vecs = stacked_handle()
    L = _lib.lib()
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=-1))
    assert load_batch(kkt, 3, ro, co, vecs)[0] == _lib.NO_DEVICE
    calls = mpc_batch_calls(L, kkt._h)
    for name, call in calls.items():
        assert call() == _lib.BADARG, name
        assert b"load first" in L.tlpk_last_error(kkt._h), name
    assert calls["start"](None) == _lib.BADARG and calls["newton"](0, None) == _lib.BADARG and calls["newton"](7) == _lib.BADARG
    assert calls["gap"](None) == _lib.BADARG and calls["targets"](par=None) == _lib.BADARG and calls["advance"](out=None) == _lib.BADARG
    for name, call in mpc_batch_calls(L, None).items():
        assert call() == _lib.BADARG, name
    kkt.close()


def test_batched_mpc_stacks_the_lps_as_the_hsd_batch_does():
    lps = small_lps()
    opt = BatchedDeviceMPC(lps, device=-1, load=False)
    assert isinstance(opt, tk.BatchedDeviceHSD) and tk.BatchedDeviceMPC is BatchedDeviceMPC
    assert opt.nlp == 3 and (opt.m, opt.n) == (10, 20)
    assert opt.row_off.tolist() == [0, 3, 8, 10] and opt.col_off.tolist() == [0, 7, 16, 20]
    assert opt.row_block.tolist() == [0] * 3 + [1] * 5 + [2] * 2
    assert np.array_equal(opt.kkt.backend_options.row_block, opt.row_block)
    for k, (A, b, c, l, u) in enumerate(lps):
        lf, uf = np.isfinite(l), np.isfinite(u)
        assert opt.p[k] == lf.sum() + uf.sum()
        assert opt.nb[k] == np.abs(b).max() and opt.nc[k] == np.abs(c).max()
        assert opt.nlz[k] == np.abs(np.where(lf, l, 0.0)).max() and opt.nuz[k] == np.abs(np.where(uf, u, 0.0)).max()
    assert np.array_equal(opt.tau, np.ones(3)) and not opt.kappa.any() and np.array_equal(opt.regP, np.ones(3)) and np.array_equal(opt.regD, np.ones(3))
    with pytest.raises(RuntimeError, match="nothing is loaded"):
        opt.optimize()
    opt.kkt.close()


def test_optimize_batch_refuses_a_mixed_list():
    lp = read_free_mps(os.path.join(GOLDEN, "lpex_opt.mps"))
    with pytest.raises(ValueError, match="mix"):
        tk.Model.optimize_batch([tk.Model(lp, algorithm="mpc"), tk.Model(lp, algorithm="hsd")], device=-1)
    with pytest.raises(ValueError, match="mix"):
        tk.Model.optimize_batch([tk.Model(lp), tk.Model(lp, algorithm="mpc")], device=-1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the float64 stand-in: the five batched calls from the unbatched ones, LP by LP
# ---------------------------------------------------------------------------------------------------------------------------------------
class MpcBatchLib(ir.StandInLib):
    """tlpk_mpc_batch_* on a stacked StandIn: LP k is a StandIn of its own whose vectors are VIEWS of the stacked ones, driven by the unbatched
    tlpk_mpc_* of StandInLib with the LP's scalars; an inactive LP is skipped and its outputs are 0."""

    def _sub(self, h, k):
        if not hasattr(h, "_subs"):
            h._subs = []
            for q in range(h.nlp):
                s = ir.StandIn(ir.segment_lp(h.lp, q, h.row_off, h.col_off))
                cs, rs = h.seg(q)
                s.v = {name: h.v[name][rs if name in ir.ROW_NAMES else cs] for name in ir.NAMES}
                h._subs.append(s)
        s = h._subs[k]
        if h.lu is not None:                                       # the factor of the stack's last update, block k
            s.D, s.lu = h.D[h.seg(k)[0]], [h.lu[k]]
        return s

    def tlpk_mpc_batch_start(self, h, out):
        o, one = ir._arr(out, h.nlp), np.zeros(1)
        h.lu = None
        for k in range(h.nlp):
            self.tlpk_mpc_start(self._sub(h, k), pd(one)); o[k] = one[0]
        return 0

    def _per_lp(self, h, active, out, width, fn):
        act, o, tmp = ir._arr(active, h.nlp, np.uint8), (ir._arr(out, width * h.nlp) if width else None), np.zeros(max(width, 1))
        for k in range(h.nlp):
            if width:
                o[width * k:width * (k + 1)] = 0.0
            if act[k]:
                fn(self._sub(h, k), k, pd(tmp))
                if width:
                    o[width * k:width * (k + 1)] = tmp[:width]
        return 0

    def tlpk_mpc_batch_newton(self, h, mode, active, gmu, out):
        g = ir._arr(gmu, h.nlp)
        return self._per_lp(h, active, out, 2, lambda s, k, o: self.tlpk_mpc_newton(s, int(mode), float(g[k]), o))

    def tlpk_mpc_batch_gap(self, h, active, ap, ad, out):
        p, d = ir._arr(ap, h.nlp), ir._arr(ad, h.nlp)
        return self._per_lp(h, active, out, 2, lambda s, k, o: self.tlpk_mpc_gap(s, float(p[k]), float(d[k]), o))

    def tlpk_mpc_batch_targets(self, h, active, par):
        q = ir._arr(par, 4 * h.nlp)
        return self._per_lp(h, active, None, 0, lambda s, k, o: self.tlpk_mpc_targets(s, *(float(x) for x in q[4 * k:4 * k + 4])))

    def tlpk_mpc_batch_advance(self, h, active, ap, ad, out):
        p, d = ir._arr(ap, h.nlp), ir._arr(ad, h.nlp)
        return self._per_lp(h, active, out, 1, lambda s, k, o: self.tlpk_mpc_advance(s, float(p[k]), float(d[k]), o))


def standin_batch(lps, options=None):
    """BatchedDeviceMPC on the stand-in: the analysis of the real constructor, the stacked StandIn in the handle's place."""
    opt = BatchedDeviceMPC([(p.A, p.b, p.c, p.l, p.u) for p in lps], load=False, device=-1, options=options)
    opt.kkt.close()
    stacked = ir.LPData(opt.A, opt._b, opt._c, opt._l, opt._u)
    opt.kkt, opt.L, opt.loaded = _Holder(ir.StandIn(stacked, opt.row_off, opt.col_off)), MpcBatchLib(), True
    return opt


def test_the_batched_loop_reproduces_device_mpc_on_the_stand_in():
    """The mask logic of the host loop: three LPs that need different numbers of iterations and corrections in one batch, each held to its own
    `DeviceMPC` run on the stand-in -- status, niter, timers, objectives, x and y are EQUAL."""
    names = ["1x1", "33x257", "rows"]
    lps = [lp_of(s) for s in names]
    opt = standin_batch(lps).optimize()
    niters = []
    for k, lp in enumerate(lps):
        one = _standin_loop(DeviceMPC, lp, None).optimize()
        print(names[k], one.status, one.niter, one.timers, "| batch", opt.status[k], int(opt.niter[k]), opt.timers_of(k))
        assert opt.status[k] == one.status and opt.niter[k] == one.niter
        got = opt.timers_of(k)
        assert {key: got[key] for key in one.timers} == one.timers
        assert opt.primal_objective[k] == one.primal_objective and opt.dual_objective[k] == one.dual_objective
        assert np.array_equal(opt._get(k, 0), one._get(0, one.n)) and np.array_equal(opt._get(k, 5), one._get(5, one.m))
        assert opt.mu[k] == one.mu and opt.alpha_p[k] == one.alpha_p and opt.alpha_d[k] == one.alpha_d
        assert opt.solution(k)["status"] == one.status
        niters.append(one.niter)
    assert len(set(niters)) > 1 and max(niters) > 0, "bad test input: the LPs leave the batch together"
    assert not opt.active.any()


def test_the_stand_in_loop_honours_per_lp_options():
    class Two(Options):
        IterationsLimit = 2

    lps = [lp_of("33x257"), lp_of("rows")]
    opt = standin_batch(lps, options=[Two(), Options()]).optimize()
    alone = _standin_loop(DeviceMPC, lps[1], None).optimize()
    assert opt.status[0] == "Trm_IterationLimit" and opt.niter[0] == 2 and opt.timers_of(0)["n_update"] == 3
    assert alone.niter > 2, "bad test input"
    assert opt.status[1] == alone.status and opt.niter[1] == alone.niter and np.array_equal(opt._get(1, 0), alone._get(0, alone.n))


# ---------------------------------------------------------------------------------------------------------------------------------------
# per-call checks: stand-in and GPU
# ---------------------------------------------------------------------------------------------------------------------------------------
class MpcDriver(Driver):
    """test_ipm_kernels.Driver for DeviceMPC with the row_block a one-LP batch gives its handle."""

    def __init__(self, kind, lp):
        if kind == "cpu":
            Driver.__init__(self, kind, lp, cls=DeviceMPC)
            return
        self.kind, self.lp = kind, lp
        self.loop = DeviceMPC(lp.A, lp.b, lp.c, lp.l, lp.u, device=0, pair_solves=False, row_block=np.zeros(lp.m, dtype=np.int64))
        self.sym = self.loop.kkt
        self.L, self.h = self.loop.L, self.loop.kkt._h


class MpcBatchDriver:
    def __init__(self, kind, names):
        self.kind, self.names = kind, list(names)
        self.lps = [lp_of(s) for s in names]
        if kind == "cpu":
            self.loop = standin_batch(self.lps)
        else:
            self.loop = BatchedDeviceMPC([(p.A, p.b, p.c, p.l, p.u) for p in self.lps], device=0)
        lo = self.loop
        self.L, self.h, self.ro, self.co, self.nlp = lo.L, lo.kkt._h, lo.row_off, lo.col_off, lo.nlp

    def read(self):
        return ir.read_all(self.L, self.h, int(self.ro[-1]), int(self.co[-1]))

    def goto(self, count):
        """The loop's own state after the starting point and `count` iterations (every LP iterated, whatever its status)."""
        lo = self.loop
        lo._init_state()
        act = lo.active; act[:] = True
        with np.errstate(all="ignore"):
            lo.compute_starting_point()
            for _ in range(count):
                lo.compute_residuals(act); lo.update_solver_status(act)
                lo.compute_step(act)
            lo.compute_residuals(act)

    def close(self):
        if self.kind == "gpu":
            self.loop.kkt.close()


def trial_box(vecs, lp, ap_, ad_):
    """tmin, tmax at the 30 % / 70 % points of the products the targets kernel forms: all three branches occur."""
    vals = np.concatenate([((vecs[x] + ap_ * vecs[dx]) * (vecs[z] + ad_ * vecs[dz]))[fl != 0]
                           for x, z, dx, dz, fl in (("xl", "zl", "dxl", "dzl", lp.lf), ("xu", "zu", "dxu", "dzu", lp.uf))])
    return (float(np.quantile(vals, 0.3)), float(np.quantile(vals, 0.7))) if vals.size >= 3 else (0.1, 10.0)


def mpcb_sequence(bd, tab, off=None):
    """Every batched MPC call once, with scalars that differ between the LPs; LP `off` (an index, or None) is inactive in every masked call.
    Active LPs: the restatement per segment.  The inactive LP: every readable vector bit-unchanged, outputs 0."""
    L, h, lo, B, lps = bd.L, bd.h, bd.loop, bd.nlp, bd.lps
    ident = np.array([float(list(SHAPES).index(name)) for name in bd.names])
    out = np.zeros(16 * B)
    act = np.ones(B, dtype=np.uint8)
    if off is not None:
        act[off] = 0
    last = [None]

    def call(name, fn, width, check):
        pre = last[0] if last[0] is not None else bd.read()
        out[:] = 7.0
        assert fn() == _lib.OK, name
        post = last[0] = bd.read()
        for k, lpname in enumerate(bd.names):
            a, b_ = ir.segment(pre, k, bd.ro, bd.co), ir.segment(post, k, bd.ro, bd.co)
            o = out[width * k:width * (k + 1)].copy()
            rep = ir.Report(f"{name} LP {lpname}")
            if act[k]:
                check(k, a, b_, o, rep)
            else:
                rep.exact("outputs of an inactive LP are 0", o, np.zeros(width))
                for key in ir.NAMES:
                    rep.exact(f"inactive: {key} untouched", a[key], b_[key])
            tab.add(f"{name}[{lpname}]" + ("" if act[k] else " off"), rep)
        return post

    def newton(mode, gmu):
        g = np.ascontiguousarray(gmu, dtype=np.float64)

        def check(k, a, b_, o, rep):
            sc = np.array(MPC_SC); sc[6] = g[k]
            ir.check_newton(lps[k], a, b_, mode, sc, o, rep, mpc=True)
        call(f"mpcb_newton{mode}", lambda: L.tlpk_mpc_batch_newton(h, mode, pu8(act), pd(g), pd(out)), 2, check)
        o2 = out[:2 * B].reshape(B, 2)
        return np.minimum(1.0, o2[:, 0]), np.minimum(1.0, o2[:, 1])

    mu = lo.mu.copy()
    regP, regD = np.ascontiguousarray((2.0 + ident) * SQRT_EPS * 1e3), np.ascontiguousarray((3.0 + ident) * SQRT_EPS * 1e3)
    fail = C.c_int64(-7)
    all_on = np.ones(B, dtype=np.uint8)
    assert L.tlpk_ipm_batch_factor(h, pu8(all_on), pd(regP), pd(regD), C.byref(fail)) == _lib.OK and fail.value == -1
    ap, ad = newton(0, np.zeros(B))
    ap, ad = np.ascontiguousarray((0.9 - 0.01 * ident) * ap), np.ascontiguousarray((0.6 + 0.01 * ident) * ad)      # ap != ad, per LP
    call("mpcb_gap", lambda: L.tlpk_mpc_batch_gap(h, pu8(act), pd(ap), pd(ad), pd(out)), 2,
         lambda k, a, b_, o, r: ir.check_mpc_gap(lps[k], a, b_, ap[k], ad[k], o, r))
    ap, ad = newton(1, (0.2 + 0.01 * ident) * mu)
    par = np.zeros((B, 4))
    par[:, 0], par[:, 1] = np.minimum(0.8 * ap + 0.3, 1.0), np.minimum(0.5 * ad + 0.3, 1.0)
    for k in range(B):
        par[k, 2:] = trial_box(ir.segment(last[0], k, bd.ro, bd.co), lps[k], par[k, 0], par[k, 1])
    cnts = {}
    call("mpcb_targets", lambda: L.tlpk_mpc_batch_targets(h, pu8(act), pd(par)), 0,
         lambda k, a, b_, o, r: cnts.__setitem__(k, ir.check_targets(lps[k], a, b_, par[k, 0], par[k, 1], par[k, 2], par[k, 3], None, r, call="mpc_targets")))
    for k, cnt in cnts.items():
        if min((lps[k].lf != 0).sum(), (lps[k].uf != 0).sum()) >= 3:
            assert all(min(c) > 0 for c in cnt), f"bad test input: LP {bd.names[k]}: the targets' branches occur {cnt} times"
    newton(2, np.zeros(B))
    call("batch_accept", lambda: L.tlpk_ipm_batch_accept(h, pu8(act)), 0, lambda k, a, b_, o, r: ir.check_accept(a, b_, r, batched=True))
    ap, ad = np.ascontiguousarray((0.45 - 0.01 * ident) * ap), np.ascontiguousarray((0.3 + 0.01 * ident) * ad)
    call("mpcb_advance", lambda: L.tlpk_mpc_batch_advance(h, pu8(act), pd(ap), pd(ad), pd(out)), 1,
         lambda k, a, b_, o, r: ir.check_advance(lps[k], a, b_, ap[k], ad[k], o, r))


PER_CALL = ["1x1", "33x257", "17x16385"]          # one block; two workgroups and a lane group with one live row; 65 blocks: the finalize lane's second trip


@pytest.mark.parametrize("kind", DRIVERS)
@pytest.mark.parametrize("count", [0, 3], ids=["start", "it3"])
def test_batched_calls_against_long_double(count, kind):
    tab = Table(kind, "mpcb", f"it{count}")
    bd = MpcBatchDriver(kind, PER_CALL)
    try:
        bd.goto(count)
        mpcb_sequence(bd, tab)
    finally:
        bd.close()
    tab.done()


@pytest.mark.parametrize("kind", DRIVERS)
def test_the_starting_point_is_the_unbatched_one(kind):
    """x, xl, xu, zl, zu, y of every LP of the batch against tlpk_mpc_start on that LP alone (a stacked factorisation rounds differently:
    1e-10 relative, the figure of tests/test_mpc_device.py); the returned xl'zl + xu'zu to the same figure."""
    bd = MpcBatchDriver(kind, PER_CALL)
    try:
        out = np.zeros(bd.nlp)
        assert bd.L.tlpk_mpc_batch_start(bd.h, pd(out)) == _lib.OK
        got = bd.read()
        for k, name in enumerate(bd.names):
            drv = Driver(kind, bd.lps[k], cls=DeviceMPC)
            try:
                one = np.zeros(1)
                drv.ok(drv.L.tlpk_mpc_start(drv.h, pd(one)))
                want, mine = drv.read(), ir.segment(got, k, bd.ro, bd.co)
            finally:
                drv.close()
            for key in ir.ITER:
                err = np.abs(mine[key] - want[key]).max() / max(1.0, np.abs(want[key]).max())
                print(f"MPCB start {kind} {name:9s} {key:3s} {err:.3e}")
                assert err <= 1e-10, (name, key)
            assert abs(out[k] - one[0]) <= 1e-10 * max(1.0, abs(one[0])), name
            assert (mine["xl"][bd.lps[k].lf != 0] > 0).all() and (mine["zu"][bd.lps[k].uf != 0] > 0).all()
    finally:
        bd.close()


@pytest.mark.parametrize("kind", DRIVERS)
def test_an_inactive_lp_is_not_touched(kind):
    """The middle LP sits out of newton (all three modes), gap, targets, accept and advance after one iteration of its own (its iterate, accepted
    direction and candidate are not zero): bit-unchanged, outputs 0; the others are restated as usual."""
    tab = Table(kind, "mpcb", "off")
    bd = MpcBatchDriver(kind, PER_CALL)
    try:
        bd.goto(1)
        pre = ir.segment(bd.read(), 1, bd.ro, bd.co)
        assert all(pre[key].any() for key in ("x", "dx", "dzl", "cx", "y", "dy")), "bad test input"
        mpcb_sequence(bd, tab, off=1)
        post = ir.segment(bd.read(), 1, bd.ro, bd.co)
        for key in ir.ITER + ir.ACC + ir.CAND:
            assert np.array_equal(pre[key].view(np.uint64), post[key].view(np.uint64)), key
    finally:
        bd.close()
    tab.done()


@pytest.mark.parametrize("kind", DRIVERS)
@pytest.mark.parametrize("shape", ["1x1", "33x257"])
def test_a_batch_of_one_equals_the_unbatched_calls(shape, kind):
    """After every one of the five calls every vector code of the one-LP batch equals the unbatched call's on a DeviceMPC handle with the same
    row_block, bit for bit, as do the returned scalars.  tlpk_ipm_batch_accept copies where tlpk_ipm_accept swaps: the candidate is left out
    after it."""
    lp = lp_of(shape)
    tab = Table(kind, shape, "mpcb1")
    drv, bd = MpcDriver(kind, lp), MpcBatchDriver(kind, [shape])
    try:
        L, h, Lb, hb = drv.L, drv.h, bd.L, bd.h
        one = np.ones(1, dtype=np.uint8); fail = C.c_int64(0)
        o, ob = np.zeros(16), np.zeros(16)
        skip = set()
        arr = lambda *v: np.array(v, dtype=np.float64)                # noqa: E731

        def same(name, width):
            rep = ir.Report(name)
            rep.exact("outputs", o[:width], ob[:width])
            va, vb = drv.read(), bd.read()
            for key in ir.NAMES:
                if key not in skip:
                    rep.exact(key, va[key], vb[key])
            tab.add(name, rep)
            return va
        drv.ok(L.tlpk_mpc_start(h, pd(o))); drv.ok(Lb.tlpk_mpc_batch_start(hb, pd(ob))); same("start", 1)
        drv.ok(L.tlpk_ipm_residuals(h, 1.0, pd(o))); drv.ok(Lb.tlpk_ipm_batch_residuals(hb, pd(arr(1.0)), pd(ob))); same("residuals", 13)
        mu = o[8] / drv.loop.p
        regP, regD = 0.1, 0.05
        drv.ok(L.tlpk_ipm_factor(h, regP, regD)); drv.ok(Lb.tlpk_ipm_batch_factor(hb, pu8(one), pd(arr(regP)), pd(arr(regD)), C.byref(fail))); same("factor", 0)
        drv.ok(L.tlpk_mpc_newton(h, 0, 0.0, pd(o))); drv.ok(Lb.tlpk_mpc_batch_newton(hb, 0, pu8(one), pd(arr(0.0)), pd(ob))); same("newton0", 2)
        ap, ad = 0.9 * min(1.0, o[0]), 0.6 * min(1.0, o[1])
        drv.ok(L.tlpk_mpc_gap(h, ap, ad, pd(o))); drv.ok(Lb.tlpk_mpc_batch_gap(hb, pu8(one), pd(arr(ap)), pd(arr(ad)), pd(ob))); same("gap", 2)
        gmu = 0.2 * mu
        drv.ok(L.tlpk_mpc_newton(h, 1, gmu, pd(o))); drv.ok(Lb.tlpk_mpc_batch_newton(hb, 1, pu8(one), pd(arr(gmu)), pd(ob))); vecs = same("newton1", 2)
        ap, ad = min(1.0, o[0]), min(1.0, o[1])
        ap_, ad_ = min(0.8 * ap + 0.3, 1.0), min(0.5 * ad + 0.3, 1.0)
        tmin, tmax = trial_box(vecs, lp, ap_, ad_)
        o[:] = 0.0; ob[:] = 0.0
        drv.ok(L.tlpk_mpc_targets(h, ap_, ad_, tmin, tmax)); drv.ok(Lb.tlpk_mpc_batch_targets(hb, pu8(one), pd(arr(ap_, ad_, tmin, tmax)))); same("targets", 0)
        drv.ok(L.tlpk_mpc_newton(h, 2, 0.0, pd(o))); drv.ok(Lb.tlpk_mpc_batch_newton(hb, 2, pu8(one), pd(arr(0.0)), pd(ob))); same("newton2", 2)
        skip |= set(ir.CAND)
        drv.ok(L.tlpk_ipm_accept(h)); drv.ok(Lb.tlpk_ipm_batch_accept(hb, pu8(one))); same("accept", 0)
        ap, ad = 0.45 * ap, 0.3 * ad
        drv.ok(L.tlpk_mpc_advance(h, ap, ad, pd(o))); drv.ok(Lb.tlpk_mpc_batch_advance(hb, pu8(one), pd(arr(ap)), pd(arr(ad)), pd(ob))); same("advance", 1)
    finally:
        drv.close(); bd.close()
    tab.done()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the loop, held to DeviceMPC's own record of each LP
# ---------------------------------------------------------------------------------------------------------------------------------------
def single(d, system="K1", options=None, **kw):
    """One LP through its own DeviceMPC: the record the batch is held to (the fields of test_hsd_batch.single)."""
    opt = DeviceMPC(d.A, d.b, d.c, d.l, d.u, c0=d.c0, objsense_min=d.objsense, device=0, system=system, options=options, **kw).optimize()
    rec = dict(status=opt.status, niter=opt.niter, zp=opt.primal_objective, zd=opt.dual_objective, rho=opt.rho, timers=dict(opt.timers),
               x=opt._get(0, opt.n), y=opt._get(5, opt.m), zl=opt._get(3, opt.n))
    opt.kkt.close()
    return rec


_cache = {}


def example_runs(system):
    """The four example LPs and their own DeviceMPC records (computed once per system, never modified)."""
    if system not in _cache:
        ds = [golden(name) for name in EXAMPLES]
        _cache[system] = (ds, [single(d, system) for d in ds])
    return _cache[system]


def check_lpex_opt(opt, k, system):
    ds, recs = example_runs(system)
    close_to(of_batch(opt, k), recs[0], 1e-9, 1e-6 if system == "K1" else 1e-5)
    assert opt.status[k] == "Trm_Optimal"
    assert abs(opt.solution(k)["z_primal"] - 1.5) <= 100 * SQRT_EPS


def batch_records(ds, **kw):
    opt = BatchedDeviceMPC(ds, device=0, **kw).optimize()
    recs = [of_batch(opt, k) for k in range(len(ds))]
    opt.kkt.close()
    return recs


@pytest.mark.gpu
@pytest.mark.parametrize("system", ["K1", "K2"])
def test_a_batch_of_one_is_device_mpc_bit_for_bit(system):
    from test_ipm_harness import random_feasible_lp
    d = standard_form(random_feasible_lp(300, 700, 5, ineq=True))
    rb = np.zeros(d.A.shape[0], dtype=np.int64)                    # the batch's default row_block, given to both
    one = single(d, system, row_block=rb)
    opt = BatchedDeviceMPC([d], system=system, device=0).optimize()
    b = of_batch(opt, 0)
    print(system, one["status"], one["niter"], b["niter"], one["timers"], b["timers"])
    assert one["status"] == "Trm_Optimal", "bad test input"
    assert b["status"] == one["status"] and b["niter"] == one["niter"]
    assert b["timers"]["n_update"] == one["timers"]["n_update"] and b["timers"]["n_solve"] == one["timers"]["n_solve"]
    assert b["zp"] == one["zp"] and b["zd"] == one["zd"]
    assert np.array_equal(b["x"], one["x"]) and np.array_equal(b["y"], one["y"])
    assert opt.solution(0)["z_primal"] == one["zp"]                # tau = 1
    opt.kkt.close()


@pytest.mark.gpu
@pytest.mark.parametrize("system", ["K1", "K2"])
def test_mixed_outcomes_in_one_batch(system):
    ds, recs = example_runs(system)
    opt = BatchedDeviceMPC(ds, system=system, device=0).optimize()
    vtol = 1e-6 if system == "K1" else 1e-5
    print(system, [r["niter"] for r in recs])
    for k, name in enumerate(EXAMPLES):
        print(system, name)
        assert recs[k]["status"] == EXAMPLE_STATUS[k], "bad test input"
        close_to(of_batch(opt, k), recs[k], 1e-9, vtol)
    check_lpex_opt(opt, 0, system)
    assert not opt.active.any()
    opt.kkt.close()


def boundary_runs():
    if "boundary" not in _cache:
        ds = boundary_lps()
        _cache["boundary"] = (ds, [single(d) for d in ds])
    return _cache["boundary"]


@pytest.mark.gpu
def test_segment_boundaries():
    ds, recs = boundary_runs()
    for r in recs:
        assert r["status"] == "Trm_Optimal", "bad test input"
    got = _cache["boundary_batch"] = batch_records(ds)
    for k in range(len(ds)):
        close_to(got[k], recs[k], 1e-8, 1e-6, niter_tol=1)


@pytest.mark.gpu
def test_batches_are_deterministic_and_independent_of_their_order():
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
    opt = BatchedDeviceMPC(ds, device=0).optimize()
    print({k: (opt.status[k], int(opt.niter[k]), opt.timers_of(k)) for k in range(3)})
    sb = opt.solution(0)
    check_retry_run(opt.timers_of(0), sb["status"], sb["z_primal"], BUMP_OPT)
    assert opt.timers_of(1)["n_bump"] == 0
    check_lpex_opt(opt, 1, "K1")
    ss = opt.solution(2)
    assert ss["status"] == "Trm_Optimal"
    assert abs(ss["z_primal"] - STAIR25_OPT) <= 1e-6 * (1 + abs(STAIR25_OPT)) and abs(ss["z_dual"] - STAIR25_OPT) <= 1e-6 * (1 + abs(STAIR25_OPT))
    assert max(ss["rho"]) <= SQRT_EPS
    opt.kkt.close()


@pytest.mark.gpu
def test_an_lp_at_its_iteration_limit_does_not_sink_the_batch():
    from test_ipm_harness import random_feasible_lp

    class TwoIterations(Options):
        IterationsLimit = 2

    d = standard_form(random_feasible_lp(81, 200, 23))
    ds, recs = example_runs("K1")
    opt = BatchedDeviceMPC([d, ds[0]], options=[TwoIterations(), Options()], device=0).optimize()
    print({k: (opt.status[k], int(opt.niter[k]), opt.timers_of(k)) for k in range(2)})
    assert opt.status[0] == "Trm_IterationLimit" and opt.niter[0] == 2
    assert opt.timers_of(0)["n_update"] == 3                       # the starting point + 2
    check_lpex_opt(opt, 1, "K1")
    assert opt.niter[1] > 2 and opt.timers_of(1)["n_update"] > 3
    assert opt.last_update_rc == _lib.OK                           # the updates after LP 0 left ran with its block parked
    opt.kkt.close()


@pytest.mark.gpu
def test_reload_equals_a_fresh_batch():
    ds, _ = example_runs("K1")
    ds = [ds[0], ds[3], golden("stair25")]
    opt = BatchedDeviceMPC(ds, device=0).optimize()
    rng = np.random.default_rng(3)
    c2 = opt._c * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, opt.n))
    opt.reload(c=c2).optimize()
    fresh = BatchedDeviceMPC([(d.A, d.b, c2[opt.col_off[k]:opt.col_off[k + 1]], d.l, d.u, d.c0, d.objsense) for k, d in enumerate(ds)], device=0).optimize()
    for k in range(3):
        a, b = of_batch(opt, k), of_batch(fresh, k)
        assert a["status"] == b["status"] and a["niter"] == b["niter"] and a["zp"] == b["zp"] and a["zd"] == b["zd"] and a["timers"] == b["timers"]
        for key in ("x", "y", "zl"):
            assert np.array_equal(a[key], b[key]), key
    assert opt.status[0] == "Trm_Optimal"
    opt.kkt.close(); fresh.kkt.close()


@pytest.mark.gpu
def test_model_optimize_batch_with_mpc_models():
    paths = [os.path.join(GOLDEN, name + ".mps") for name in EXAMPLES]
    own = [tk.Model.load(p, algorithm="mpc", device=0).optimize() for p in paths]
    models = tk.Model.optimize_batch([tk.Model.load(p, algorithm="mpc") for p in paths], device=0)
    print([(m.status, m.inner is None) for m in own])
    for a, b in zip(models, own):
        assert a.status == b.status
        assert (a.inner is None) == (b.inner is None)            # (a model presolve alone solves never reaches the batch)
        for f in ("objective_value", "dual_objective_value"):
            za, zb = getattr(a, f)(), getattr(b, f)()
            assert (za == zb) or abs(za - zb) <= 1e-9 * (1 + abs(zb)), (f, za, zb)
    assert [m.status for m in own] == EXAMPLE_STATUS
