"""Per-call tests of the interior-point kernels against long double (tests/ipm_reference.py holds the restatement, the rule
|device - r| <= 2 K u M and its derivation).  The loop-level tests (test_hsd_device.py, test_mpc_device.py, test_hsd_batch.py) compare a few
scalars and x, y after whole iterations; a converging loop forgives a wrong entry of a direction, a clamp on the wrong side, a dropped row.
Here every C entry point of the device-resident loops is called on its own and every vector it writes is read back (tlpk_ipm_get, codes
0 .. 35) and compared, entry by entry, with the long-double value of the same formula on the device's own inputs.

Every check is written once and runs on two drivers: the float64 stand-in of tests/ipm_reference.py (unmarked, any machine) and libtlpk.so on
the GPU (`-m gpu`).  States come from the real loops (compute_residuals / compute_step): the starting point, after 3 iterations, and the first
iteration with mu < 1e-7 (else the last one before optimality); the long LP: the starting point and one iteration.  The calls then take scalars
of the test's choosing.  Every figure is printed before it is asserted (lines "IPMK ..."; profiles/ipm_kernel_checks.txt is such a run on an
MI355X).  test_mutation_* shows on the stand-in that each of ten deliberate defects breaks a bound.

The KKT check (solve_stats of tests/backward_error.py, unchanged) runs where the factored matrix has at most 64 rows: its allowances are dense.
It is asserted for every solve but the one inside a mode 2 call, whose solution cannot be reconstructed (NOT_MET in tests/ipm_reference.py:
the figure is printed).  The targets' three branches are asserted wherever an LP has three bounded entries per side (not the 1 x 1 LP)."""
import ctypes as C
import functools
import re
import zlib

import numpy as np
import pytest
import scipy.sparse as sp

import ipm_reference as ir
import tulip_jl_amd as tk
from backward_error import Allowances, System, blocks_of, restate, solve_stats
from tulip_jl_amd import _lib
from tulip_jl_amd.hsd_batch import BatchedDeviceHSD
from tulip_jl_amd.hsd_device import SQRT_EPS, DeviceHSD, Options
from tulip_jl_amd.mpc_device import DeviceMPC

GPU = pytest.param("gpu", marks=pytest.mark.gpu)
DRIVERS = ["cpu", GPU]
RATIO = 8.0                 # the solves: omega_unit <= RATIO max(restatement's, 1)   (tests/backward_error.py, "WHY 8")
LONG_N, LONG_M = 262145 + 256, 32768 + 9
pd = _lib.as_pd


# ---------------------------------------------------------------------------------------------------------------------------------
# LPs: free, lower-only, upper-only and boxed columns, nonzero bounds, primal and dual feasible by construction
# ---------------------------------------------------------------------------------------------------------------------------------
KINDS8 = "FLLBLLUB"         # columns 254 .. 257 (and 16382 .. 16385): U, B, F, L -- one of each kind on a workgroup boundary
KINDS_SMALL = "BLUFLBU"     # fewer than 8 columns


def make_lp(m, n, seed, per_col=2, special_rows=(), one_per_col=False):
    rng = np.random.default_rng(seed)
    if one_per_col:                                              # the long LP: one entry per column, rows of about n / m entries -- A D A' is diagonal
        rows, cols = np.arange(n) % m, np.arange(n)
    elif special_rows:                                           # the first rows hold exactly the given numbers of entries; the others cover every column
        k = len(special_rows)
        rows = [np.full(c, i) for i, c in enumerate(special_rows)] + [k + rng.integers(0, m - k, n)]
        cols = [rng.choice(n, size=c, replace=False) for c in special_rows] + [np.arange(n)]
        extra = k + np.arange(m - k)                             # every other row holds an entry
        rows, cols = np.concatenate(rows + [extra]), np.concatenate(cols + [extra % n])
    else:
        k = min(per_col, m)
        rows = np.concatenate([rng.choice(m, size=k, replace=False) for _ in range(n)]) if n <= 4096 else (rng.integers(0, m, n)[:, None] + np.arange(k)[None, :] * (1 + m // 3)).ravel() % m
        cols = np.repeat(np.arange(n), k)
        rows, cols = np.concatenate([rows, np.arange(m)]), np.concatenate([cols, np.arange(m) % n])      # no empty row
    vals = rng.uniform(0.5, 2.0, rows.size) * rng.choice([-1.0, 1.0], rows.size)
    A = sp.coo_matrix((vals, (rows, cols)), shape=(m, n)).tocsc()
    A.sum_duplicates(); A.sort_indices()
    kinds = np.array(list((KINDS_SMALL * 2)[:n] if n < 8 else (KINDS8 * (n // 8 + 1))[:n]))
    F, Lo, Up, B = kinds == "F", kinds == "L", kinds == "U", kinds == "B"
    l, u = np.full(n, -np.inf), np.full(n, np.inf)
    l[Lo | B] = rng.uniform(-1.0, 1.0, int((Lo | B).sum()))
    u[B] = l[B] + rng.uniform(0.3, 1.0, int(B.sum()))
    u[Up] = rng.uniform(2.0, 3.0, int(Up.sum()))
    x0 = rng.standard_normal(n) * 3.0
    x0[Lo] = l[Lo] + rng.uniform(2.0, 6.0, int(Lo.sum())); x0[Up] = u[Up] - rng.uniform(2.0, 6.0, int(Up.sum()))
    x0[B] = l[B] + (u[B] - l[B]) * rng.uniform(0.2, 0.8, int(B.sum()))
    z0 = rng.uniform(0.1, 1.0, n)
    z0[Up] *= -1.0; z0[B] *= rng.choice([-1.0, 1.0], int(B.sum())); z0[F] = 0.0
    b = A @ x0
    c = A.T @ rng.standard_normal(m) + z0
    return ir.LPData(A, b, c, l, u)


SHAPES = {
    "1x1": lambda: make_lp(1, 1, 1),
    "31x255": lambda: make_lp(31, 255, 2),                       # one workgroup of a column kernel and of the row kernel, both short by one
    "32x256": lambda: make_lp(32, 256, 3),                       # exactly one
    "33x257": lambda: make_lp(33, 257, 4),                       # two of each; m = 8 k + 1: a lane group with one live row
    "rows": lambda: make_lp(12, 40, 5, special_rows=(1, 8, 9, 17)),      # the lane loop's trip counts
    "9x16384": lambda: make_lp(9, 16384, 6),                     # 64 blocks: one trip of the finalize lane
    "17x16385": lambda: make_lp(17, 16385, 7),                   # 65 blocks: its second trip
    "long": lambda: make_lp(LONG_M, LONG_N, 8, one_per_col=True),        # second grid-stride trip of the column kernels under the 1024-block clamp
}
STATES = {name: (("start", "it1") if name == "long" else ("start", "it3", "late")) for name in SHAPES}
CASES = [(s, st) for s in SHAPES for st in STATES[s]]


@functools.lru_cache(maxsize=None)
def lp_of(name):
    return SHAPES[name]()


# ---------------------------------------------------------------------------------------------------------------------------------
# drivers: the real loop classes on libtlpk.so (gpu) or on the stand-in (cpu)
# ---------------------------------------------------------------------------------------------------------------------------------
class _Holder:
    def __init__(self, h):
        self._h = h


def _standin_loop(cls, lp, mut):
    """The loop class on the stand-in: everything but the handle comes from the class's own `_init_loop` (what its constructor runs after the load)."""
    o = object.__new__(cls)
    o.kkt, o.L = _Holder(ir.StandIn(lp, mut=mut)), ir.StandInLib()
    o.pair_solves, o.overlap_root = False, False
    o.m, o.n, o.opt = lp.m, lp.n, Options()
    o._b, o._c, o._l, o._u, o.c0, o.objsense = lp.b, lp.c, lp.l, lp.u, 0.0, True
    o._init_loop()
    return o


class Driver:
    """One LP on one handle: the loop object, the library (or its stand-in) and the handle the calls take."""

    def __init__(self, kind, lp, cls=DeviceHSD, mut=None, dense=False):
        self.kind, self.lp = kind, lp
        if kind == "cpu":
            self.loop = _standin_loop(cls, lp, mut)
            self.sym = None if dense else tk.setup(lp.A, tk.K1(), tk.Backend(device=-1))      # the analysis: the permutation and blocks of the KKT check
        else:
            A = lp.A.toarray() if dense else lp.A
            self.loop = cls(A, lp.b, lp.c, lp.l, lp.u, device=0, pair_solves=False, dense=dense)
            self.sym = self.loop.kkt
        self.L, self.h = self.loop.L, self.loop.kkt._h

    def read(self):
        return ir.read_all(self.L, self.h, self.lp.m, self.lp.n)

    def ok(self, rc):
        assert rc == _lib.OK, f"return code {rc}"

    def goto(self, state):
        """The loop's own state after `state` iterations from the starting point (deterministic: a replay gives the same bits)."""
        if state == "late":
            n, found = 0, None
            self._start()
            while n < 60:
                self.loop.compute_residuals(); self.loop.update_solver_status()
                if self.loop.status != "Trm_Unknown":
                    found = max(n - 1, 0); break                 # the last iteration before the stopping test fires
                self.loop.compute_step(); n += 1
                if self.loop.mu < 1e-7:
                    found = n; break
            count = n if found is None else found
        else:
            count = {"start": 0, "it1": 1, "it3": 3}[state]
        self._start()
        for _ in range(count):
            self.loop.compute_residuals(); self.loop.update_solver_status()
            self.loop.compute_step()
        self.loop.compute_residuals()
        return count

    def _start(self):
        lo = self.loop
        self.ok(self.L.tlpk_ipm_reset(self.h))
        lo.regP = lo.regD = lo.regG = 1.0
        if isinstance(lo, DeviceMPC):
            lo.tau, lo.kappa = 1.0, 0.0
            lo.compute_starting_point()
        else:
            lo.tau = lo.kappa = 1.0

    def close(self):
        if self.kind == "gpu":
            self.loop.kkt.close()


class Table:
    """The figures of one test: printed as they come, asserted at the end."""

    def __init__(self, who, shape, state):
        self.head, self.bad = f"IPMK {who:3s} {shape:9s} {state:5s}", []

    def add(self, call, rep):
        label, worst = max(rep.rows, key=lambda r: r[1]) if rep.rows else ("-", 0.0)
        print(f"{self.head} {call:22s} worst |dev - r| / (K u M) = {worst:9.3e}  ({label}; {len(rep.rows)} outputs)")
        self.bad += rep.bad

    def note(self, call, what, value, limit):
        print(f"{self.head} {call:22s} {what} = {value:9.3e}  (limit {limit:g})")
        if not value <= limit:
            self.bad.append(f"{call}: {what} = {value:.3e} > {limit:g}")

    def done(self):
        assert not self.bad, "\n".join([self.head] + self.bad[:40])


class SolveCheck:
    """tests/backward_error.py's solve_stats for the solves inside the calls: omega_unit <= 8 max(restatement's, 1)."""

    def __init__(self, drv):
        self.drv, self.on = drv, drv.sym is not None and drv.lp.m <= ir.SOLVE_CHECK_MAX_N
        if self.on:
            self.perm, self.blocks = drv.sym.symbolic("perm"), blocks_of(drv.sym)

    def factored(self, vecs):
        if self.on:
            self.data = (vecs["theta"].copy(), vecs["regP"].copy(), vecs["regD"].copy())
            if self.drv.kind == "gpu":
                from emulate import panels_to_dense_L
                self.Ldev = np.tril(panels_to_dense_L(self.drv.sym, self.drv.sym.factor_panels()))

    def check(self, tab, call, xip, xid, dx, dy, mode=None):
        if not self.on:
            return
        system = System("k1", self.drv.lp.A, self.perm, self.data + (np.asarray(xip, np.float64), np.asarray(xid, np.float64)))
        Lr, wr = restate(system, self.blocks)
        ref = solve_stats(Allowances(system, Lr, self.blocks), wr)["unit"]
        L = self.Ldev if self.drv.kind == "gpu" else Lr
        st = solve_stats(Allowances(system, L, self.blocks), system.permuted(dx, dy))
        limit = RATIO * max(ref, 1.0)
        if mode == 2:       # NOT_MET of tests/ipm_reference.py: the solution is reconstructed through the accepted direction's addition.  Printed, not asserted.
            print(f"{tab.head} {call:22s} mode 2 KKT solve omega_unit of the reconstructed solution (restatement {ref:.2e}) = {st['unit']:9.3e}  "
                  f"(limit {limit:g}: {'met' if st['unit'] <= limit else 'not met'}; not asserted)")
            return
        tab.note(call, f"KKT solve omega_unit (restatement {ref:.2e})", st["unit"], limit)


def pick_targets(vecs, lp, a_):
    """mu_l, mu_u at the 30 % / 70 % points of the products the targets kernel forms: all three branches occur on both sides."""
    vals = []
    for x, z, dx, dz, fl in (("xl", "zl", "dxl", "dzl", lp.lf), ("xu", "zu", "dxu", "dzu", lp.uf)):
        vals.append(((vecs[x] + a_ * vecs[dx]) * (vecs[z] + a_ * vecs[dz]))[fl != 0])
    allv = np.concatenate(vals)
    if allv.size == 0:
        return 0.1, 10.0
    if allv.size < 3:
        return float(allv.min()) * 1.5 + 0.01, float(allv.max()) * 2.0 + 1.0
    lo, hi = np.quantile(allv, 0.3), np.quantile(allv, 0.7)
    return float(lo), float(hi)


def hsd_sequence(drv, tab, paired_replay=None):
    """Every HSD call once, from the loop's current state, each checked against the restatement.  Returns the trace [(call, outputs, vectors)]."""
    lp, L, h, lo = drv.lp, drv.L, drv.h, drv.loop
    out, sc = np.zeros(16), np.zeros(8)
    tau, kappa, regG = 0.83 * lo.tau, 1.21 * lo.kappa, 0.37
    regP, regD = 2.0 * max(lo.regP, SQRT_EPS), 3.0 * max(lo.regD, SQRT_EPS)
    sol = SolveCheck(drv)
    trace, last = [], [None]

    def call(name, fn, check):
        pre = last[0] if last[0] is not None else drv.read()     # nothing ran since the previous call's read-back
        drv.ok(fn())
        post = last[0] = drv.read()
        rep = ir.Report(name)
        res = check(pre, post, rep)
        tab.add(name, rep)
        trace.append((name, out.copy(), post))
        return post, res

    post, _ = call("residuals", lambda: L.tlpk_ipm_residuals(h, tau, pd(out)), lambda a, b, r: ir.check_residuals(lp, a, b, tau, out, r))
    cx, dualsum, xz = out[4], out[5] + out[6] - out[7], out[8]
    rg, mu = kappa + (cx - dualsum), (xz + tau * kappa) / (lo.p + 1)
    post, _ = call("factor", lambda: L.tlpk_ipm_factor(h, regP, regD), lambda a, b, r: ir.check_factor(lp, a, b, regP, regD, r))
    sol.factored(post)
    if paired_replay is None:
        post, _ = call("hsolve", lambda: L.tlpk_ipm_hsolve(h, pd(out)), lambda a, b, r: ir.check_hsolve(lp, a, b, out, r))
        sol.check(tab, "hsolve", lp.b, post["hxid"], post["hx"], post["hy"])
        h0 = float(out[0]) + kappa / tau + regG
        sc[:] = (tau, kappa, h0, rg, -tau * kappa, 0.0, 0.0, 0.0)
        post, s = call("newton0", lambda: L.tlpk_ipm_newton(h, 0, pd(sc), pd(out)), lambda a, b, r: ir.check_newton(lp, a, b, 0, sc, out, r))
        sol.check(tab, "newton0", s["xip"], s["xid"], s["dx"], s["dy"], s["mode"])
        trace[-1] = ("newton0", np.concatenate([out[:3], [h0]]), post)
    else:
        sc[:] = (tau, kappa, regG, rg, -tau * kappa, 0.0, 0.0, 0.0)
        post, s = call("hsolve_newton", lambda: L.tlpk_ipm_hsolve_newton(h, pd(sc), pd(out)), lambda a, b, r: ir.check_hsolve_newton(lp, a, b, sc, out, r))
        sol.check(tab, "hsolve_newton h", lp.b, post["hxid"], post["hx"], post["hy"])
        sol.check(tab, "hsolve_newton d", s["xip"], s["xid"], s["dx"], s["dy"], s["mode"])
        # the header's promise: the same arithmetic as tlpk_ipm_hsolve + tlpk_ipm_newton(mode 0), bit for bit on vectors and scalars
        name, o_single, v_single = paired_replay
        rep = ir.Report("paired = single calls")
        rep.exact("dtau, dkappa, step, h0", out[:4], o_single)
        for key in ir.NAMES:
            if key not in ir.CAND:                               # neither path writes the candidate; the first pass's later calls left theirs in it
                rep.exact(key, post[key], v_single[key])
        tab.add("paired = hsolve+newton0", rep)
        return trace
    dtau, dkappa, h0 = float(out[0]), float(out[1]), float(sc[2])
    eta, gmu = 0.93, 0.07 * mu
    sc[:] = (tau, kappa, h0, eta * rg, -tau * kappa + gmu - dtau * dkappa, eta, gmu, 0.0)
    post, s = call("newton1", lambda: L.tlpk_ipm_newton(h, 1, pd(sc), pd(out)), lambda a, b, r: ir.check_newton(lp, a, b, 1, sc, out, r))
    sol.check(tab, "newton1", s["xip"], s["xid"], s["dx"], s["dy"], s["mode"])
    dtau, dkappa, step = float(out[0]), float(out[1]), float(out[2])
    a_ = min(1.0, 1.7 * min(step, 1.0))
    mu_l, mu_u = pick_targets(post, lp, a_)
    post, cnt = call("targets", lambda: L.tlpk_ipm_targets(h, a_, mu_l, mu_u, pd(out)), lambda a, b, r: ir.check_targets(lp, a, b, a_, a_, mu_l, mu_u, out, r))
    if min((lp.lf != 0).sum(), (lp.uf != 0).sum()) >= 3:
        assert all(min(c) > 0 for c in cnt), f"bad test input: the targets' branches (below, inside, above) occur {cnt} times on the lower / upper side"
    vt = 0.01 * mu
    delta = (float(out[0]) + float(out[1]) + vt) / (lo.p + 1)
    sc[:] = (tau, kappa, h0, 0.0, vt - delta, 0.0, 0.0, delta)
    post, s = call("newton2", lambda: L.tlpk_ipm_newton(h, 2, pd(sc), pd(out)), lambda a, b, r: ir.check_newton(lp, a, b, 2, sc, out, r))
    sol.check(tab, "newton2", s["xip"], s["xid"], s["dx"], s["dy"], s["mode"])
    out[:] = 0.0
    call("accept", lambda: L.tlpk_ipm_accept(h), lambda a, b, r: ir.check_accept(a, b, r))
    alpha = 0.5 * min(1.0, float(step))
    call("advance", lambda: L.tlpk_ipm_advance(h, alpha, pd(out)), lambda a, b, r: ir.check_advance(lp, a, b, alpha, alpha, out, r))
    return trace


def run_hsd(kind, shape, state, mut=None):
    lp = lp_of(shape)
    drv = Driver(kind, lp, mut=mut)
    tab = Table(kind, shape, state)
    try:
        drv.goto(state)
        trace = hsd_sequence(drv, tab)
        single = next(t for t in trace if t[0] == "newton0")
        drv.goto(state)                                          # the same state again: the paired call from it
        hsd_sequence(drv, tab, paired_replay=single)
    finally:
        drv.close()
    return tab


@pytest.mark.parametrize("kind", DRIVERS)
@pytest.mark.parametrize("shape,state", CASES, ids=[f"{a}-{b}" for a, b in CASES])
def test_hsd_calls(shape, state, kind):
    """residuals, factor, hsolve, newton 0 / 1 / 2, targets, accept, advance, and hsolve_newton = hsolve + newton(0) bit for bit."""
    run_hsd(kind, shape, state).done()


# ---------------------------------------------------------------------------------------------------------------------------------
# Mehrotra
# ---------------------------------------------------------------------------------------------------------------------------------
MPC_SC = (1.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0)              # tau = 1, eta = 1, delta = 0, dtau = 0: what tlpk_mpc_newton passes to the shared kernels


def mpc_sequence(drv, tab):
    lp, L, h, lo = drv.lp, drv.L, drv.h, drv.loop
    out = np.zeros(16)
    sol = SolveCheck(drv)
    regP, regD = 2.0 * max(lo.regP, SQRT_EPS), 3.0 * max(lo.regD, SQRT_EPS)
    last = [None]

    def call(name, fn, check):
        pre = last[0] if last[0] is not None else drv.read()
        drv.ok(fn())
        post = last[0] = drv.read()
        rep = ir.Report(name)
        res = check(pre, post, rep)
        tab.add(name, rep)
        return post, res

    def newton(mode, gmu):
        sc = np.array(MPC_SC); sc[6] = gmu
        post, s = call(f"mpc_newton{mode}", lambda: L.tlpk_mpc_newton(h, mode, gmu, pd(out)), lambda a, b, r: ir.check_newton(lp, a, b, mode, sc, out, r, mpc=True))
        sol.check(tab, f"mpc_newton{mode}", s["xip"], s["xid"], s["dx"], s["dy"], s["mode"])
        return min(1.0, float(out[0])), min(1.0, float(out[1]))

    call("residuals", lambda: L.tlpk_ipm_residuals(h, 1.0, pd(out)), lambda a, b, r: ir.check_residuals(lp, a, b, 1.0, out, r))
    mu = float(out[8]) / max(lo.p, 1)
    post, _ = call("factor", lambda: L.tlpk_ipm_factor(h, regP, regD), lambda a, b, r: ir.check_factor(lp, a, b, regP, regD, r))
    sol.factored(post)
    ap, ad = newton(0, 0.0)
    ap, ad = 0.9 * ap, 0.6 * ad                                  # ap != ad
    call("mpc_gap", lambda: L.tlpk_mpc_gap(h, ap, ad, pd(out)), lambda a, b, r: ir.check_mpc_gap(lp, a, b, ap, ad, out, r))
    ap, ad = newton(1, 0.2 * mu)
    ap_, ad_ = min(0.8 * ap + 0.3, 1.0), min(0.5 * ad + 0.3, 1.0)
    post = last[0]
    vals = np.concatenate([((post[x] + ap_ * post[dx]) * (post[z] + ad_ * post[dz]))[fl != 0]
                           for x, z, dx, dz, fl in (("xl", "zl", "dxl", "dzl", lp.lf), ("xu", "zu", "dxu", "dzu", lp.uf))])
    tmin, tmax = (float(np.quantile(vals, 0.3)), float(np.quantile(vals, 0.7))) if vals.size >= 3 else (0.1, 10.0)
    _, cnt = call("mpc_targets", lambda: L.tlpk_mpc_targets(h, ap_, ad_, tmin, tmax),
                  lambda a, b, r: ir.check_targets(lp, a, b, ap_, ad_, tmin, tmax, None, r, call="mpc_targets"))
    if min((lp.lf != 0).sum(), (lp.uf != 0).sum()) >= 3:
        assert all(min(c) > 0 for c in cnt), f"bad test input: the targets' branches occur {cnt} times"
    newton(2, 0.0)
    call("accept", lambda: L.tlpk_ipm_accept(h), lambda a, b, r: ir.check_accept(a, b, r))
    ap, ad = 0.45 * ap, 0.3 * ad
    call("mpc_advance", lambda: L.tlpk_mpc_advance(h, ap, ad, pd(out)), lambda a, b, r: ir.check_advance(lp, a, b, ap, ad, out, r))


def run_mpc(kind, shape, state, mut=None):
    drv = Driver(kind, lp_of(shape), cls=DeviceMPC, mut=mut)
    tab = Table(kind, shape, "m-" + state)
    try:
        drv.goto(state)
        mpc_sequence(drv, tab)
    finally:
        drv.close()
    return tab


MPC_CASES = [(s, st) for s in SHAPES if s != "long" for st in ("start", "it3", "late")] + [("long", "start")]


@pytest.mark.parametrize("kind", DRIVERS)
@pytest.mark.parametrize("shape,state", MPC_CASES, ids=[f"{a}-{b}" for a, b in MPC_CASES])
def test_mpc_calls(shape, state, kind):
    """tlpk_mpc_gap, tlpk_mpc_targets, tlpk_mpc_advance with ap != ad; tlpk_mpc_newton: both steps to the boundary, recovery with dtau = 0."""
    run_mpc(kind, shape, state).done()


@pytest.mark.parametrize("kind", DRIVERS)
def test_residuals_on_a_dense_matrix_handle(kind):
    """The aty / ax branch of ipm_res_col and ipm_res_row: A'y and A x come from the GEMV kernels (K = m and K = n)."""
    rng = np.random.default_rng(12)
    sparse = make_lp(20, 50, 9, per_col=3)
    Ad = sparse.A.toarray() + 0.1 * rng.standard_normal((20, 50))
    x0 = np.where(np.isfinite(sparse.l), sparse.l, np.where(np.isfinite(sparse.u), sparse.u - 3.0, 0.0)) + 1.0
    x0 = np.where(np.isfinite(sparse.u), np.minimum(x0, sparse.u - 0.1), x0)
    lp = ir.LPData(Ad, Ad @ x0, sparse.c, sparse.l, sparse.u, dense=True)
    drv = Driver(kind, lp, dense=True)
    out = np.zeros(16)
    try:
        for state in ("start", "it3"):
            tab = Table(kind, "dense", state)
            drv.goto(state)
            tau = 0.77 * drv.loop.tau
            pre = drv.read()
            drv.ok(drv.L.tlpk_ipm_residuals(drv.h, tau, pd(out)))
            rep = ir.Report("residuals")
            ir.check_residuals(lp, pre, drv.read(), tau, out, rep)
            tab.add("residuals", rep)
            tab.done()
    finally:
        drv.close()


# the cuts of the two GEMV kernels (tests/test_dense_shapes.py names them): one row and one column; m = 2 under n mod 4 = 1; a second trip of
# k_dense_gemv_t's lane loop with an odd m, n = 3 (one live wave short of a workgroup); the second 512-row workgroup of k_dense_gemv_n with 8 live
# threads, 2 chunks of 9 | 8; 964 chunks of 17 columns, the last of 14
DENSE_GEMV_SHAPES = [(1, 1), (2, 17), (129, 3), (513, 17), (16, 16385)]


@pytest.mark.parametrize("kind", DRIVERS)
@pytest.mark.parametrize("m,n", DENSE_GEMV_SHAPES, ids=[f"{m}x{n}" for m, n in DENSE_GEMV_SHAPES])
def test_residuals_on_a_dense_matrix_handle_at_the_gemv_cuts(m, n, kind):
    """The same branch (D == nullptr in k_dense_gemv_t / k_dense_gemv_n) at the shapes where those kernels change behaviour, m > n among them."""
    rng = np.random.default_rng(100 * m + n)
    sparse = make_lp(m, n, 13, per_col=3)
    Ad = sparse.A.toarray() + 0.1 * rng.standard_normal((m, n))
    x0 = np.where(np.isfinite(sparse.l), sparse.l, np.where(np.isfinite(sparse.u), sparse.u - 3.0, 0.0)) + 1.0
    x0 = np.where(np.isfinite(sparse.u), np.minimum(x0, sparse.u - 0.1), x0)
    lp = ir.LPData(Ad, Ad @ x0, sparse.c, sparse.l, sparse.u, dense=True)
    drv = Driver(kind, lp, dense=True)
    out = np.zeros(16)
    try:
        for state in ("start", "it3"):
            tab = Table(kind, f"d{m}x{n}"[:9], state)
            drv.goto(state)
            tau = 0.77 * drv.loop.tau
            pre = drv.read()
            drv.ok(drv.L.tlpk_ipm_residuals(drv.h, tau, pd(out)))
            rep = ir.Report("residuals")
            ir.check_residuals(lp, pre, drv.read(), tau, out, rep)
            tab.add("residuals", rep)
            tab.done()
    finally:
        drv.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# batched
# ---------------------------------------------------------------------------------------------------------------------------------
BATCH = ["1x1", "33x257", "17x16385", "long"]


class BatchDriver:
    def __init__(self, kind, names, mut=None):
        self.kind, self.names = kind, list(names)
        lps = [lp_of(s) for s in names]
        tup = [(p.A, p.b, p.c, p.l, p.u) for p in lps]
        if kind == "cpu":
            self.loop = BatchedDeviceHSD(tup, load=False, device=-1)
            lo = self.loop
            self.stacked = ir.LPData(lo.A, lo._b, lo._c, lo._l, lo._u)
            lo.kkt, lo.L, lo.loaded = _Holder(ir.StandIn(self.stacked, lo.row_off, lo.col_off, mut=mut)), ir.StandInLib(), True
        else:
            self.loop = BatchedDeviceHSD(tup, device=0)
        lo = self.loop
        self.L, self.h, self.ro, self.co, self.nlp = lo.L, lo.kkt._h, lo.row_off, lo.col_off, lo.nlp
        self.lps = lps

    def read(self):
        return ir.read_all(self.L, self.h, int(self.ro[-1]), int(self.co[-1]))

    def goto(self, count):
        lo = self.loop
        assert self.L.tlpk_ipm_reset(self.h) == _lib.OK
        lo._init_state()
        act = lo.active; act[:] = True
        with np.errstate(all="ignore"):
            for _ in range(count):
                lo.compute_residuals(act); lo.update_solver_status(act)
                lo.compute_step(act)
            lo.compute_residuals(act)

    def close(self):
        if self.kind == "gpu":
            self.loop.kkt.close()


class BatchSolveCheck:
    """SolveCheck for every LP of a SMALL batch (the dense factor of the whole stack is read back): LP k's rows of the stacked permutation, the
    diagonal blocks among them and its block of the factor are that LP's own factored system -- the stack is block diagonal."""

    def __init__(self, bd):
        self.bd, self.part = bd, {}
        assert int(bd.ro[-1]) <= ir.SOLVE_CHECK_MAX_N
        if bd.kind == "gpu":
            kkt = bd.loop.kkt
            perm, blocks = kkt.symbolic("perm"), blocks_of(kkt)
            for k in range(bd.nlp):
                pos = np.nonzero((perm >= bd.ro[k]) & (perm < bd.ro[k + 1]))[0]
                where = {int(p): i for i, p in enumerate(pos)}
                bl = [(where[c0], w) for c0, w in blocks if c0 in where]
                assert all(where.get(c0 + w - 1) == where[c0] + w - 1 for c0, w in blocks if c0 in where) and sum(w for _, w in bl) == pos.size, "a diagonal block spans two LPs"
                self.part[k] = (pos, perm[pos] - bd.ro[k], bl)
        else:
            for k, lp in enumerate(bd.lps):
                kkt = tk.setup(lp.A, tk.K1(), tk.Backend(device=-1))
                self.part[k] = (None, kkt.symbolic("perm"), blocks_of(kkt))

    def factored(self, post):
        self.data = {k: tuple(ir.segment(post, k, self.bd.ro, self.bd.co)[key].copy() for key in ("theta", "regP", "regD")) for k in range(self.bd.nlp)}
        if self.bd.kind == "gpu":
            from emulate import panels_to_dense_L
            kkt = self.bd.loop.kkt
            self.L = np.tril(panels_to_dense_L(kkt, kkt.factor_panels()))

    def check(self, tab, call, k, xip, xid, dx, dy, mode=None):
        pos, perm, blocks = self.part[k]
        one = SolveCheck.__new__(SolveCheck)
        one.on, one.perm, one.blocks, one.data = True, perm, blocks, self.data[k]
        one.drv = _Holder(None); one.drv.kind, one.drv.lp = self.bd.kind, self.bd.lps[k]
        if self.bd.kind == "gpu":
            one.Ldev = self.L[np.ix_(pos, pos)]
        one.check(tab, call, xip, xid, dx, dy, mode)


def batch_sequence(bd, tab, off_of, restate_it=True, sol=None):
    """Every tlpk_ipm_batch_* call once with per-LP scalars; in call number q the LP `off_of(q)` (an index into bd.names, or None) is inactive.
    Returns {LP name: [(call, its outputs, its segment of every vector)]}.  restate_it = False: only the inactive LPs' checks and the trace
    (a batch whose traces are compared bit for bit with a checked one)."""
    L, h, lo, B = bd.L, bd.h, bd.loop, bd.nlp
    by_name = {name: [] for name in bd.names}
    sc, out = np.zeros((B, 8)), np.zeros(16 * B)
    ident = np.array([float(list(SHAPES).index(name)) for name in bd.names])      # scalars by the LP's identity, not its position: they differ between LPs
    tau, kappa, regG = (0.8 + 0.03 * ident) * lo.tau, (1.1 + 0.05 * ident) * lo.kappa, 0.3 + 0.02 * ident
    regP, regD = (2.0 + ident) * np.maximum(lo.regP, SQRT_EPS), (3.0 + ident) * np.maximum(lo.regD, SQRT_EPS)
    fail = C.c_int64(-7)
    ncall, last = [0], [None]

    def call(name, fn, width, check, masked=True):
        off = off_of(ncall[0]) if masked else None
        ncall[0] += 1
        act = np.ones(B, dtype=np.uint8)
        if off is not None:
            act[off] = 0
        pre = last[0] if last[0] is not None else bd.read()
        out[:] = 7.0
        assert fn(_lib.as_pu8(act)) == _lib.OK
        post = last[0] = bd.read()
        res = {}
        for k, lpname in enumerate(bd.names):
            a, b_ = ir.segment(pre, k, bd.ro, bd.co), ir.segment(post, k, bd.ro, bd.co)
            o = out[width * k:width * (k + 1)].copy()
            rep = ir.Report(f"{name} LP {lpname}")
            if act[k]:
                if restate_it or name == "batch_targets":
                    res[k] = check(k, a, b_, o, rep)
                if sol is not None and isinstance(res.get(k), dict):      # the solves of this call, LP by LP
                    if name == "batch_hsolve_newton":
                        sol.check(tab, f"{name}[{lpname}] h", k, bd.lps[k].b, b_["hxid"], b_["hx"], b_["hy"])
                    q = res[k]
                    sol.check(tab, f"{name}[{lpname}]", k, q["xip"], q["xid"], q["dx"], q["dy"], q["mode"])
            else:
                rep.exact("outputs of an inactive LP are 0", o, np.zeros(width))
                if name == "batch_factor":
                    ir.check_factor(bd.lps[k], a, b_, 0, 0, rep, active=False)
                else:
                    for key in ir.NAMES:
                        rep.exact(f"inactive: {key} untouched", a[key], b_[key])
            if rep.rows:
                tab.add(f"{name}[{lpname}]" + ("" if act[k] else " off"), rep)
            by_name[lpname].append((name, bool(act[k]), o, {key: digest(v) for key, v in b_.items()}))
        return post, res

    lps = bd.lps
    tau = np.ascontiguousarray(tau)
    _, _ = call("batch_residuals", lambda a: L.tlpk_ipm_batch_residuals(h, pd(tau), pd(out)), 13,
                lambda k, a, b_, o, r: ir.check_residuals(lps[k], a, b_, tau[k], o, r), masked=False)
    o13 = out[:13 * B].reshape(B, 13).copy()
    rg = kappa + (o13[:, 4] - (o13[:, 5] + o13[:, 6] - o13[:, 7]))
    mu = (o13[:, 8] + tau * kappa) / (lo.p + 1)
    call("batch_factor", lambda a: L.tlpk_ipm_batch_factor(h, a, pd(np.ascontiguousarray(regP)), pd(np.ascontiguousarray(regD)), C.byref(fail)), 0,
         lambda k, a, b_, o, r: ir.check_factor(lps[k], a, b_, regP[k], regD[k], r))
    assert fail.value == -1
    if sol is not None:
        sol.factored(last[0])
    for q, v in enumerate((tau, kappa, regG, rg, -tau * kappa)):
        sc[:, q] = v
    sc[:, 5:] = 0.0
    _, _ = call("batch_hsolve_newton", lambda a: L.tlpk_ipm_batch_hsolve_newton(h, a, pd(sc), pd(out)), 4,
                lambda k, a, b_, o, r: ir.check_hsolve_newton(lps[k], a, b_, sc[k], o, r))
    o4 = out[:4 * B].reshape(B, 4).copy()
    h0 = np.where(o4[:, 3] != 0, o4[:, 3], 1.0)                  # (the LP that sat out keeps a usable h0 for the later calls)
    eta, gmu = 0.9 + 0.01 * ident, (0.05 + 0.01 * ident) * mu
    for q, v in enumerate((tau, kappa, h0, eta * rg, -tau * kappa + gmu - o4[:, 0] * o4[:, 1], eta, gmu, 0.0)):
        sc[:, q] = v
    _, _ = call("batch_newton1", lambda a: L.tlpk_ipm_batch_newton(h, 1, a, pd(sc), pd(out)), 3,
                lambda k, a, b_, o, r: ir.check_newton(lps[k], a, b_, 1, sc[k], o, r))
    step = out[:3 * B].reshape(B, 3)[:, 2].copy()
    post = last[0]
    par = np.zeros((B, 3))
    for k in range(B):
        par[k, 0] = min(1.0, 1.7 * min(step[k] if step[k] > 0 else 0.5, 1.0))
        par[k, 1:] = pick_targets(ir.segment(post, k, bd.ro, bd.co), lps[k], par[k, 0])
    _, cnts = call("batch_targets", lambda a: L.tlpk_ipm_batch_targets(h, a, pd(par), pd(out)), 2,
                   lambda k, a, b_, o, r: ir.check_targets(lps[k], a, b_, par[k, 0], par[k, 0], par[k, 1], par[k, 2], o, r))
    for k, cnt in cnts.items():
        if min((lps[k].lf != 0).sum(), (lps[k].uf != 0).sum()) >= 3:
            assert all(min(c) > 0 for c in cnt), f"bad test input: LP {bd.names[k]}: the targets' branches occur {cnt} times"
    t2 = out[:2 * B].reshape(B, 2).copy()
    vt = 0.01 * mu
    delta = (t2[:, 0] + t2[:, 1] + vt) / (lo.p + 1)
    for q, v in enumerate((tau, kappa, h0, 0.0, vt - delta, 0.0, 0.0, delta)):
        sc[:, q] = v
    call("batch_newton2", lambda a: L.tlpk_ipm_batch_newton(h, 2, a, pd(sc), pd(out)), 3,
         lambda k, a, b_, o, r: ir.check_newton(lps[k], a, b_, 2, sc[k], o, r))
    call("batch_accept", lambda a: L.tlpk_ipm_batch_accept(h, a), 0, lambda k, a, b_, o, r: ir.check_accept(a, b_, r, batched=True))
    alpha = np.ascontiguousarray(0.5 * np.minimum(1.0, np.where(step > 0, step, 0.5)) * (1.0 - 0.05 * ident))
    call("batch_advance", lambda a: L.tlpk_ipm_batch_advance(h, a, pd(alpha), pd(out)), 1,
         lambda k, a, b_, o, r: ir.check_advance(lps[k], a, b_, alpha[k], alpha[k], o, r))
    # predictor alone (mode 0 of tlpk_ipm_batch_newton) from the moved point's own right-hand sides
    for q, v in enumerate((tau, kappa, h0, rg, -tau * kappa, 0.0, 0.0, 0.0)):
        sc[:, q] = v
    call("batch_newton0", lambda a: L.tlpk_ipm_batch_newton(h, 0, a, pd(sc), pd(out)), 3,
         lambda k, a, b_, o, r: ir.check_newton(lps[k], a, b_, 0, sc[k], o, r))
    return by_name


def digest(v):
    """Stands for the bits of a vector (the traces of the long LP would hold gigabytes otherwise)."""
    v = np.ascontiguousarray(v)
    return zlib.crc32(v), int(v.view(np.uint64).sum(dtype=np.uint64)), v.size


def same_traces(tab, what, ta, tb):
    rep = ir.Report(what)
    assert [t[:2] for t in ta] == [t[:2] for t in tb]
    for (name, act, oa, va), (_, _, ob, vb) in zip(ta, tb):
        rep.exact(f"{name} outputs", oa, ob)
        for key in ir.NAMES:
            rep._push(f"{name} {key} (bits)", 0.0 if va[key] == vb[key] else float("inf"))
    tab.add(what, rep)


@pytest.mark.parametrize("kind", DRIVERS)
@pytest.mark.parametrize("count", [0, 1], ids=["start", "it1"])
def test_batch_calls_and_their_independence_of_order_and_composition(count, kind):
    """One batch of the 1 x 1, the 257-column, the 16385-column and the long LP, and the same LPs in another order: every call against the
    restatement per LP; an inactive LP (one in every call, chosen by identity) is not written and returns 0; an LP's outputs and vectors are
    the same bits in either order, and the 257-column LP's in a batch of its own."""
    tab = Table(kind, "batch", f"it{count}")
    traces = []
    for names in (BATCH, [BATCH[2], BATCH[3], BATCH[1], BATCH[0]], [BATCH[1]]):
        bd = BatchDriver(kind, names)
        try:
            bd.goto(count)
            # call number q leaves out LP BATCH[q mod 4] -- by identity, so that an LP sees the same masks in every batch
            traces.append(batch_sequence(bd, tab, lambda q, names=names: names.index(BATCH[q % 4]) if BATCH[q % 4] in names else None,
                                         restate_it=names is BATCH))
        finally:
            bd.close()
    for name in BATCH:
        same_traces(tab, f"order: LP {name}", traces[0][name], traces[1][name])
    same_traces(tab, f"composition: LP {BATCH[1]} alone", traces[0][BATCH[1]], traces[2][BATCH[1]])
    tab.done()


@pytest.mark.parametrize("kind", DRIVERS)
@pytest.mark.parametrize("count", [0, 3], ids=["start", "it3"])
def test_batch_solves_with_an_inactive_lp(count, kind):
    """The KKT check on the batched calls, LP by LP, in a batch small enough for its dense factor: the solves go through scratch vectors and
    the active LPs take their segments, while one LP sits out of every call."""
    names = ["1x1", "33x257", "rows"]
    tab = Table(kind, "batch3", f"it{count}")
    bd = BatchDriver(kind, names)
    try:
        bd.goto(count)
        batch_sequence(bd, tab, lambda q: q % 3, sol=BatchSolveCheck(bd))
    finally:
        bd.close()
    tab.done()


@pytest.mark.parametrize("kind", DRIVERS)
@pytest.mark.parametrize("shape,state", [("1x1", "it3"), ("33x257", "it3"), ("17x16385", "start")])
def test_a_batch_of_one_equals_the_unbatched_calls(shape, state, kind):
    """Call by call and vector by vector, bit for bit (test_hsd_batch.py compares the end of a whole run).  tlpk_ipm_batch_accept copies where
    tlpk_ipm_accept swaps the two buffers: after it the CANDIDATE differs by design (include/tlpk.h) and is left out, as is what later calls
    leave in it."""
    lp = lp_of(shape)
    count = {"start": 0, "it3": 3}[state]
    tab = Table(kind, shape, "b1-" + state)
    drv, bd = Driver(kind, lp), BatchDriver(kind, [shape])
    try:
        drv.goto(state); bd.goto(count)
        assert drv.loop.tau == bd.loop.tau[0] and drv.loop.kappa == bd.loop.kappa[0], "the two loops left the same state"
        L, h, Lb, hb = drv.L, drv.h, bd.L, bd.h
        one = np.ones(1, dtype=np.uint8); fail = C.c_int64(0)
        o, ob, sc = np.zeros(16), np.zeros(16), np.zeros(8)
        tau, kappa, regG = 0.83 * drv.loop.tau, 1.21 * drv.loop.kappa, 0.37
        regP, regD = 2.0 * max(drv.loop.regP, SQRT_EPS), 3.0 * max(drv.loop.regD, SQRT_EPS)
        skip = set(ir.CAND)                                      # the loops' own accepts left different candidates behind (swap / copy)

        def same(name, width):
            rep = ir.Report(name)
            rep.exact("outputs", o[:width], ob[:width])
            va, vb = drv.read(), bd.read()
            for key in ir.NAMES:
                if key not in skip:
                    rep.exact(key, va[key], vb[key])
            tab.add(name, rep)
        arr = lambda *v: np.array(v, dtype=np.float64)                # noqa: E731
        drv.ok(L.tlpk_ipm_residuals(h, tau, pd(o))); drv.ok(Lb.tlpk_ipm_batch_residuals(hb, pd(arr(tau)), pd(ob))); same("residuals", 13)
        rg, mu = kappa + (o[4] - (o[5] + o[6] - o[7])), (o[8] + tau * kappa) / (drv.loop.p + 1)
        drv.ok(L.tlpk_ipm_factor(h, regP, regD)); drv.ok(Lb.tlpk_ipm_batch_factor(hb, _lib.as_pu8(one), pd(arr(regP)), pd(arr(regD)), C.byref(fail))); same("factor", 0)
        sc[:] = (tau, kappa, regG, rg, -tau * kappa, 0, 0, 0)
        drv.ok(L.tlpk_ipm_hsolve_newton(h, pd(sc), pd(o))); drv.ok(Lb.tlpk_ipm_batch_hsolve_newton(hb, _lib.as_pu8(one), pd(sc), pd(ob))); same("hsolve_newton", 4)
        dtau, dkappa, h0 = o[0], o[1], o[3]
        eta, gmu = 0.93, 0.07 * mu
        sc[:] = (tau, kappa, h0, eta * rg, -tau * kappa + gmu - dtau * dkappa, eta, gmu, 0)
        drv.ok(L.tlpk_ipm_newton(h, 1, pd(sc), pd(o))); drv.ok(Lb.tlpk_ipm_batch_newton(hb, 1, _lib.as_pu8(one), pd(sc), pd(ob))); same("newton1", 3)
        a_ = min(1.0, 1.7 * min(float(o[2]), 1.0))
        mu_l, mu_u = pick_targets(drv.read(), lp, a_)
        drv.ok(L.tlpk_ipm_targets(h, a_, mu_l, mu_u, pd(o))); drv.ok(Lb.tlpk_ipm_batch_targets(hb, _lib.as_pu8(one), pd(arr(a_, mu_l, mu_u)), pd(ob))); same("targets", 2)
        vt = 0.01 * mu
        delta = (o[0] + o[1] + vt) / (drv.loop.p + 1)
        sc[:] = (tau, kappa, h0, 0, vt - delta, 0, 0, delta)
        drv.ok(L.tlpk_ipm_newton(h, 2, pd(sc), pd(o))); drv.ok(Lb.tlpk_ipm_batch_newton(hb, 2, _lib.as_pu8(one), pd(sc), pd(ob))); skip.clear(); same("newton2", 3)
        skip |= set(ir.CAND)
        drv.ok(L.tlpk_ipm_accept(h)); drv.ok(Lb.tlpk_ipm_batch_accept(hb, _lib.as_pu8(one))); same("accept", 0)
        drv.ok(L.tlpk_ipm_advance(h, 0.4, pd(o))); drv.ok(Lb.tlpk_ipm_batch_advance(hb, _lib.as_pu8(one), pd(arr(0.4)), pd(ob))); same("advance", 1)
        sc[:] = (tau, kappa, h0, rg, -tau * kappa, 0, 0, 0)
        drv.ok(L.tlpk_ipm_newton(h, 0, pd(sc), pd(o))); drv.ok(Lb.tlpk_ipm_batch_newton(hb, 0, _lib.as_pu8(one), pd(sc), pd(ob))); same("newton0", 3)
    finally:
        drv.close(); bd.close()
    tab.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# the window itself
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_codes_have_names_and_lengths():
    assert _lib.IPM_GET_NAMES == ir.NAMES and len(ir.NAMES) == 36
    assert {ir.NAMES[c] for c in _lib.IPM_GET_ROWS} == set(ir.ROW_NAMES)
    assert (_lib.IPM_X, _lib.IPM_DX, _lib.IPM_CX, _lib.IPM_RP, _lib.IPM_THL, _lib.IPM_XIL, _lib.IPM_THETA, _lib.IPM_REGD) == (0, 6, 12, 18, 22, 27, 33, 35)
    header = open(__file__.replace("tests/test_ipm_kernels.py", "include/tlpk.h")).read()
    assert "33-35" in header and "12-17" in header


@pytest.mark.parametrize("kind", DRIVERS)
def test_get_refuses_unknown_codes_and_wrong_lengths(kind):
    lp = lp_of("rows")
    drv = Driver(kind, lp)
    try:
        v = np.zeros(max(lp.m, lp.n) + 1)
        for code in (-1, 36, 1000):
            assert drv.L.tlpk_ipm_get(drv.h, code, pd(v), lp.n) == _lib.BADARG
        for code, name in enumerate(ir.NAMES):
            good = lp.m if name in ir.ROW_NAMES else lp.n
            assert drv.L.tlpk_ipm_get(drv.h, code, pd(v), good) == _lib.OK, name
            assert drv.L.tlpk_ipm_get(drv.h, code, pd(v), good + 1) == _lib.BADARG, name
        if kind == "gpu":                                        # DeviceHSD._get passes the codes through
            assert np.array_equal(drv.loop._get(_lib.IPM_XL, lp.n), lp.lf) and drv.loop._get(_lib.IPM_REGD, lp.m).shape == (lp.m,)
    finally:
        drv.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the checker must be able to fail: one deliberate defect at a time in the stand-in, each must break a bound
# ---------------------------------------------------------------------------------------------------------------------------------
def _caught(tab, words):
    hit = [b for b in tab.bad if any(re.match(w, b) for w in words)]              # "<call> <output>: ratio ...": the call and output the defect sits in
    print("\n".join(["caught:"] + tab.bad[:6]))
    return hit


@pytest.mark.parametrize("mut,shape,state,words", [
    ("rd_signs", "33x257", "start", ["residuals rd"]),                                       # zl and zu exchange signs in rd
    ("xxu_flag", "33x257", "it3", ["residuals out11 |(x+xu)uf|"]),                           # the |(x + xu) uflag| maximum drops its flag
    ("last_row", "33x257", "start", ["residuals rp", "residuals out0 |rp|", "residuals out5 b'y"]),      # the row kernel drops the last row of the 8 k + 1 LP
    ("second_trip", "long", "start", ["residuals out6 lz'zl", "residuals out7 uz'zu", "residuals out8 xl'zl+xu'zu"]),      # a sum drops the second grid-stride trip
    ("upper_clamp", "33x257", "start", ["targets xzl", "targets xzu"]),                      # the upper clamp of the targets uses mu_l
    ("dxl_dtau", "33x257", "start", ["newton0 dxl"]),                                        # dxl forgets dtau lz
    ("mode2_dzu", "33x257", "start", ["newton2 dzu"]),                                       # mode 2 forgets to add the accepted direction to dzu
    ("slots", "33x257", "start", ["residuals out6 lz'zl", "residuals out7 uz'zu"]),          # two result slots are swapped
])
def test_mutation_hsd(mut, shape, state, words):
    lp = lp_of(shape)
    drv = Driver("cpu", lp, mut=mut)
    tab = Table("mut", shape, state)
    drv.goto(state)
    hsd_sequence(drv, tab)
    assert _caught(tab, [re.escape(w) + ":" for w in words]), f"the mutation {mut} passes the checks of {words}"


def test_mutation_mpc_advance_uses_alpha_d_on_the_primal_side():
    drv = Driver("cpu", lp_of("33x257"), cls=DeviceMPC, mut="mpc_alpha")
    tab = Table("mut", "33x257", "m-start")
    drv.goto("start")
    mpc_sequence(drv, tab)
    assert _caught(tab, [r"mpc_advance (x|xl|xu):"])


def test_mutation_an_inactive_lps_xil_is_written():
    names = ["1x1", "33x257", "rows"]
    bd = BatchDriver("cpu", names, mut="inactive_xil")
    tab = Table("mut", "batch", "start")
    bd.goto(0)
    batch_sequence(bd, tab, lambda q: q % 3)
    assert _caught(tab, [r"batch_(hsolve_newton|newton\d) LP \S+ inactive: xil untouched \(bits\):"])


def test_the_reduction_depth_follows_the_launch():
    """blocks and trips of the formula K = K_entry + trips + 8 + ceil(blocks / 64) + 6 at the sizes the shapes are chosen for."""
    assert [ir.seg_blocks(n) for n in (1, 255, 256, 257, 16384, 16385, LONG_N)] == [1, 1, 1, 2, 64, 65, 1024]
    assert ir.depth(256, 1) == 1 + 8 + 1 + 6 and ir.depth(16385, 65) == 1 + 8 + 2 + 6 and ir.depth(LONG_N, 1024) == 2 + 8 + 16 + 6
    assert ir.depth(33, 1, per=8) == 2 + 8 + 1 + 6 and ir.depth(LONG_M, ir.seg_blocks(LONG_M), per=8) == 8 + 8 + 3 + 6
    rng = np.random.default_rng(0)
    for n, nb in ((1, 1), (257, 2), (16385, 65), (300000, 1024)):
        v = rng.standard_normal(n)
        r = v.astype(np.longdouble).sum()
        assert abs(ir.dev_sum(v, nb) - r) <= 2 * ir.depth(n, nb) * ir.U * np.abs(v).sum()
        assert ir.dev_sum(v, nb, first_trip_only=True) == ir.dev_sum(v[:nb * 256], nb)
