"""Many small LPs in one set of launches: the homogeneous self-dual loop of hsd_device.py on a STACK of LPs (DESIGN.md section 4b').

B LPs stacked into one block-diagonal matrix are an ordinary handle: with `row_block` = LP index and no linking rows the analysis is a
forest, and the level-batched factorisation / solve kernels serve every block in the launches one block needs.  What a stacked
`DeviceHSD` cannot do is iterate the LPs independently -- it has one tau, one step length, one stopping test.  Here every scalar of
`DeviceHSD.optimize` / `compute_step` is a numpy array of length B and every branch a mask; the vector work goes through the
`tlpk_ipm_batch_*` calls (include/tlpk.h), whose kernels skip the LPs a mask leaves out.  An LP leaves the active set when its status is
decided and is never touched again; with B = 1 the run is `DeviceHSD`'s bit for bit.

    opt = BatchedDeviceHSD([standard_form(lp) for lp in lps], device=0)      # or tuples (A, b, c, l, u[, c0[, objsense_min]])
    opt.optimize()
    opt.status[k], opt.niter[k], opt.primal_objective[k], opt.solution(k)
"""
import ctypes as C
import time

import numpy as np

from . import _lib
from .hsd_device import Options
from .kkt import K1, K2, Backend, DimensionMismatch, OutOfMemoryError, _raise_for, setup

_DECIDED = ("Trm_Optimal", "Trm_PrimalInfeasible", "Trm_DualInfeasible")


def _fields(lp):
    """(A, b, c, l, u, c0, objsense_min) of one entry of `lps`: a tuple, or a `standard_form` result."""
    if isinstance(lp, (tuple, list)):
        if not 5 <= len(lp) <= 7:
            raise TypeError("an LP is (A, b, c, l, u[, c0[, objsense_min]]) or a standard_form result")
        A, b, c, l, u = lp[:5]
        c0 = lp[5] if len(lp) > 5 else 0.0
        sense = lp[6] if len(lp) > 6 else True
        return A, b, c, l, u, float(c0), bool(sense)
    return lp.A, lp.b, lp.c, lp.l, lp.u, float(getattr(lp, "c0", 0.0)), bool(getattr(lp, "objsense", True))


class BatchedDeviceHSD:
    def __init__(self, lps, system="K1", options=None, load=True, **backend_kw):
        # options: one Options for every LP, or a sequence with one per LP
        # load=False: stop after the analysis (the stacking can be inspected on a machine without a GPU: device=-1)
        # backend_kw: tlpk.Backend's (device, refine, ordering, ...); row_block defaults to the LP index of every row
        import scipy.sparse as sp
        lps = list(lps)
        if not lps:
            raise ValueError("BatchedDeviceHSD needs at least one LP")
        parts = [_fields(lp) for lp in lps]
        mats = []
        for (A, *_rest) in parts:
            A = sp.csc_matrix(A) if sp.issparse(A) else sp.csc_matrix(np.asarray(A, dtype=np.float64))
            mats.append(A)
        self.nlp = B = len(parts)
        ms = np.array([A.shape[0] for A in mats], dtype=np.int64); ns = np.array([A.shape[1] for A in mats], dtype=np.int64)
        if (ms < 1).any() or (ns < 1).any():
            raise DimensionMismatch("every LP of a batch needs at least one row and one column")
        self.row_off = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
        self.col_off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        vec = lambda q, lens, what: self._stack([p[q] for p in parts], lens, what)      # noqa: E731
        self._b, self._c = vec(1, ms, "b"), vec(2, ns, "c")
        self._l, self._u = vec(3, ns, "l"), vec(4, ns, "u")
        self.c0 = np.array([p[5] for p in parts]); self.objsense = np.array([p[6] for p in parts], dtype=bool)
        self.A = sp.block_diag(mats, format="csc")
        self.A.sort_indices()
        self.row_block = np.repeat(np.arange(B, dtype=np.int64), ms)
        backend_kw.setdefault("row_block", self.row_block)
        if int(backend_kw.get("nranks", 1)) > 1 or int(backend_kw.get("ngpus", 1)) > 1 or backend_kw.get("dense_cols") is not None:
            raise ValueError("a batch of LPs needs a single-device direct handle (no nranks / ngpus > 1, no dense_cols)")
        self.kkt = setup(self.A, K2() if str(system).upper() == "K2" else K1(), Backend(**backend_kw))
        self.m, self.n = self.kkt.m, self.kkt.n
        if options is None or isinstance(options, Options) or isinstance(options, type):
            options = [options or Options()] * B
        options = list(options)
        if len(options) != B:
            raise ValueError("options: one Options object, or one per LP")
        self.opts = options
        opt_arr = lambda name: np.array([float(getattr(o, name)) for o in options])      # noqa: E731
        self._o = {name: opt_arr(name) for name in ("IterationsLimit", "TolerancePFeas", "ToleranceDFeas", "ToleranceRGap", "ToleranceIFeas",
                                                    "CorrectionLimit", "StepDampFactor", "GammaMin", "CentralityOutlierThreshold", "PRegMin", "DRegMin")}
        self.time_limit = min(float(o.TimeLimit) for o in options)               # TimeLimit is global
        self.L = _lib.lib()
        self._host_norms()
        self._init_state()
        self.last_update_rc = None
        self.loaded = False
        if load:
            self._call(self.L.tlpk_ipm_load_batch(self.kkt._h, B, _lib.as_p64(self.row_off), _lib.as_p64(self.col_off),
                                                  _lib.as_pd(self._b), _lib.as_pd(self._c), _lib.as_pd(self._l), _lib.as_pd(self._u)))
            self.loaded = True

    @staticmethod
    def _stack(vs, lens, what):
        out = []
        for k, (v, length) in enumerate(zip(vs, lens)):
            a = np.asarray(v, dtype=np.float64)
            if a.shape != (int(length),):
                raise DimensionMismatch(f"LP {k}: {what} does not match A")
            out.append(a)
        return np.ascontiguousarray(np.concatenate(out))

    def _seg(self, off, f, v):
        return np.array([f(v[off[k]:off[k + 1]]) for k in range(self.nlp)])

    def _host_norms(self):
        l, u = self._l, self._u
        lf, uf = np.isfinite(l), np.isfinite(u)
        nrm = lambda v: float(np.abs(v).max(initial=0.0))                    # noqa: E731
        cnt = lambda v: int(v.sum())                                         # noqa: E731
        self.p = self._seg(self.col_off, cnt, lf) + self._seg(self.col_off, cnt, uf)      # HSD.jl:39, per LP
        self.nb, self.nc = self._seg(self.row_off, nrm, self._b), self._seg(self.col_off, nrm, self._c)
        self.nlz, self.nuz = self._seg(self.col_off, nrm, np.where(lf, l, 0.0)), self._seg(self.col_off, nrm, np.where(uf, u, 0.0))

    def _init_state(self):
        B = self.nlp
        one = lambda: np.ones(B)                                             # noqa: E731
        self.regP, self.regD, self.regG = one(), one(), one()                # HSD.jl:50-52 (uniform within an LP)
        self.tau, self.kappa, self.mu = one(), one(), one()
        self.rg, self.h0 = np.zeros(B), np.zeros(B)
        self.niter = np.zeros(B, dtype=np.int64)
        self.status = np.array(["Trm_Unknown"] * B, dtype=object)
        self.primal_status = np.array(["Sln_Unknown"] * B, dtype=object)
        self.dual_status = np.array(["Sln_Unknown"] * B, dtype=object)
        self.active = np.zeros(B, dtype=bool)
        self.timers = {name: np.zeros(B, dtype=np.int64) for name in ("n_update", "n_solve", "n_bump", "n_paired", "max_bumps_in_a_step")}
        self.rho = np.zeros((B, 3))
        for name in ("rp_nrm", "rl_nrm", "ru_nrm", "rd_nrm", "cx", "xz", "ax_nrm", "xxl_nrm", "xxu_nrm", "delta_nrm", "dualsum", "rg_nrm",
                     "primal_objective", "dual_objective"):
            setattr(self, name, np.zeros(B))
        self.seconds = 0.0
        self._cache = {}

    def timers_of(self, k):
        """The timers of LP k as `DeviceHSD.timers` holds them."""
        return {name: int(v[k]) for name, v in self.timers.items()}

    def reload(self, b=None, c=None, l=None, u=None, c0=None):
        """New stacked vectors on the analysed handle (None = keep; bounds may change between finite and infinite): tlpk_ipm_reload
        refreshes the device copies and restores the starting point, `optimize()` then solves the new LPs."""
        new = {}
        for name, v, length in (("b", b, self.m), ("c", c, self.n), ("l", l, self.n), ("u", u, self.n)):
            if v is None:
                continue
            a = np.array(v, dtype=np.float64, order="C", copy=True)
            if a.shape != (length,):
                raise DimensionMismatch(f"reload: {name} does not match the stacked A")
            new[name] = a
        ptr = lambda name: _lib.as_pd(new[name]) if name in new else None    # noqa: E731
        self._call(self.L.tlpk_ipm_reload(self.kkt._h, ptr("b"), ptr("c"), ptr("l"), ptr("u")))
        self._b, self._c = new.get("b", self._b), new.get("c", self._c)
        self._l, self._u = new.get("l", self._l), new.get("u", self._u)
        if c0 is not None:
            self.c0 = np.broadcast_to(np.asarray(c0, dtype=np.float64), (self.nlp,)).copy()
        self._host_norms()
        self._init_state()
        return self

    def _call(self, rc):
        _raise_for(rc, self.kkt._h, "tlpk_ipm_batch: ")

    @staticmethod
    def _set(dst, mask, val):
        dst[mask] = np.asarray(val)[mask] if np.ndim(val) else val

    # HSD.jl:77-128, for the LPs of `act` (the others keep what they recorded when they left)
    def compute_residuals(self, act):
        o = np.zeros(13 * self.nlp)
        self._call(self.L.tlpk_ipm_batch_residuals(self.kkt._h, _lib.as_pd(self.tau), _lib.as_pd(o)))
        o = o.reshape(self.nlp, 13)
        for q, name in enumerate(("rp_nrm", "rl_nrm", "ru_nrm", "rd_nrm", "cx")):
            self._set(getattr(self, name), act, o[:, q])
        for q, name in ((8, "xz"), (9, "ax_nrm"), (10, "xxl_nrm"), (11, "xxu_nrm"), (12, "delta_nrm")):
            self._set(getattr(self, name), act, o[:, q])
        by, lzzl, uzzu = o[:, 5], o[:, 6], o[:, 7]
        self._set(self.dualsum, act, by + lzzl - uzzu)
        self._set(self.rg, act, self.kappa + (self.cx - self.dualsum))
        self._set(self.rg_nrm, act, np.abs(self.rg))
        self._set(self.primal_objective, act, self.cx / self.tau + self.c0)
        self._set(self.dual_objective, act, self.dualsum / self.tau + self.c0)
        self._set(self.mu, act, (self.xz + self.tau * self.kappa) / (self.p + 1))          # point.jl:45-48

    # HSD.jl:136-196
    def update_solver_status(self, act):
        o, tau = self._o, self.tau
        rho_p = np.maximum(np.maximum(self.rp_nrm / (tau * (1 + self.nb)), self.rl_nrm / (tau * (1 + self.nlz))), self.ru_nrm / (tau * (1 + self.nuz)))
        rho_d = self.rd_nrm / (tau * (1 + self.nc))
        rho_g = np.abs(self.primal_objective - self.dual_objective) / (1 + np.abs(self.dual_objective))
        pf, df = rho_p <= o["TolerancePFeas"], rho_d <= o["ToleranceDFeas"]
        optimal = pf & df & (rho_g <= o["ToleranceRGap"])
        dinf = ~optimal & (np.maximum(np.maximum(self.ax_nrm, self.xxl_nrm), self.xxu_nrm) * (self.nc / np.maximum(1.0, self.nb)) < -o["ToleranceIFeas"] * self.cx)
        pinf = ~optimal & ~dinf & (self.delta_nrm * np.maximum(np.maximum(self.nlz, self.nuz), self.nb) / np.maximum(1.0, self.nc) < self.dualsum * o["ToleranceIFeas"])
        status = np.full(self.nlp, "Trm_Unknown", dtype=object)
        primal = np.where(pf, "Sln_FeasiblePoint", "Sln_Unknown").astype(object)
        dual = np.where(df, "Sln_FeasiblePoint", "Sln_Unknown").astype(object)
        status[optimal] = "Trm_Optimal"; primal[optimal] = "Sln_Optimal"; dual[optimal] = "Sln_Optimal"
        status[dinf] = "Trm_DualInfeasible"; primal[dinf] = "Sln_InfeasibilityCertificate"
        status[pinf] = "Trm_PrimalInfeasible"; dual[pinf] = "Sln_InfeasibilityCertificate"
        self.rho[act] = np.stack([rho_p, rho_d, rho_g], axis=1)[act]
        self._set(self.status, act, status); self._set(self.primal_status, act, primal); self._set(self.dual_status, act, dual)

    def _mask(self, m):
        self._m8 = np.ascontiguousarray(m, dtype=np.uint8)
        return _lib.as_pu8(self._m8)

    def _newton(self, mode, m, xi_g, xi_tk, eta=0.0, gmu=0.0, delta=0.0):
        """step.jl:198-266 for the LPs of `m`; returns (dtau, dkappa, max step over the vector part) as arrays."""
        B = self.nlp
        sc = np.zeros((B, 8))
        for q, v in enumerate((self.tau, self.kappa, self.h0, xi_g, xi_tk, eta, gmu, delta)):
            sc[:, q] = v
        out = np.zeros((B, 3))
        self._call(self.L.tlpk_ipm_batch_newton(self.kkt._h, mode, self._mask(m), _lib.as_pd(sc), _lib.as_pd(out)))
        self.timers["n_solve"][m] += 1
        return out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy()

    def _max_step(self, a_vec, dtau, dkappa):                                # step.jl:294-306
        at = np.where(dtau < 0, -self.tau / np.where(dtau < 0, dtau, 1.0), 1.0)
        ak = np.where(dkappa < 0, -self.kappa / np.where(dkappa < 0, dkappa, 1.0), 1.0)
        return np.minimum(np.minimum(np.minimum(1.0, a_vec), at), ak)

    # step.jl:10-151 for the LPs of `act`; an LP that runs into the three-bump rule gets Trm_NumericalProblem and is parked
    def compute_step(self, act):
        o = self._o
        step = act.copy()
        self._set(self.regP, step, np.maximum(o["PRegMin"], self.regP / 10))
        self._set(self.regD, step, np.maximum(o["DRegMin"], self.regD / 10))
        self._set(self.regG, step, np.maximum(o["PRegMin"], self.regG / 10))
        step = self._factor(step)
        if not step.any():
            return step
        with np.errstate(all="ignore"):
            return self._direction_and_move(step)

    _bumped = ("regD", "regP", "regG")                                       # what a failed update multiplies by 100

    def _factor(self, step):
        """The per-LP retry loop of the update (step.jl:35-51) for the LPs of `step`; returns the LPs that hold a factor."""
        B = self.nlp
        step = step.copy()
        nbump = np.zeros(B, dtype=np.int64)
        fail = C.c_int64(-1)
        while step.any():                                                    # step.jl:35-51, per LP
            rc = self.L.tlpk_ipm_batch_factor(self.kkt._h, self._mask(step), _lib.as_pd(self.regP), _lib.as_pd(self.regD), C.byref(fail))
            self.last_update_rc = rc
            if rc == _lib.OK:
                self.timers["n_update"][step] += 1
                break
            if rc != _lib.NOT_POSDEF:
                self._call(rc)
            k = int(fail.value)
            bad = np.zeros(B, dtype=bool)
            if 0 <= k < B and step[k]:
                bad[k] = True                                                # the update reports one failure at a time
            else:
                bad[:] = step                                                # the pivot cannot be attributed: every LP of the update retries
            for name in self._bumped:
                getattr(self, name)[bad] *= 100
            nbump[bad] += 1
            self.timers["n_bump"][bad] += 1
            gone = bad & ~(nbump < 3)                                        # step.jl:51 (the reference's off-by-one is kept)
            self.status[gone] = "Trm_NumericalProblem"
            step &= ~gone
        self.timers["max_bumps_in_a_step"] = np.maximum(self.timers["max_bumps_in_a_step"], nbump)
        return step

    def _direction_and_move(self, step):
        o, B = self._o, self.nlp
        # h-system (step.jl:56-76) and predictor: independent right-hand sides, one pass over the factor
        sc = np.zeros((B, 8))
        sc[:, 0], sc[:, 1], sc[:, 2], sc[:, 3], sc[:, 4] = self.tau, self.kappa, self.regG, self.rg, -self.tau * self.kappa
        out = np.zeros((B, 4))
        self._call(self.L.tlpk_ipm_batch_hsolve_newton(self.kkt._h, self._mask(step), _lib.as_pd(sc), _lib.as_pd(out)))
        self.timers["n_solve"][step] += 2; self.timers["n_paired"][step] += 1
        dtau, dkappa, av = out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy()
        self._set(self.h0, step, out[:, 3])
        alpha = self._max_step(av, dtau, dkappa)
        # (1 - alpha) ** 2 through Python's float power, as hsd_device.py computes it: numpy squares by multiplying
        sq = np.array([(1.0 - a) ** 2 for a in alpha.tolist()])
        gamma = sq * np.minimum(1 - alpha, o["GammaMin"])
        eta = 1 - gamma
        # corrector (second-order terms from the predictor direction, which it overwrites)
        dtau, dkappa, av = self._newton(1, step, eta * self.rg, -self.tau * self.kappa + gamma * self.mu - dtau * dkappa, eta=eta, gmu=gamma * self.mu)
        alpha = self._max_step(av, dtau, dkappa)
        ncor = 0
        cor = step & (ncor < o["CorrectionLimit"]) & (alpha < 0.999)
        while cor.any():                                                     # step.jl:104-136: while ANY LP still corrects
            a_ = alpha.copy()
            ncor += 1
            # compute_higher_corrector, step.jl:325-401
            beta = o["CentralityOutlierThreshold"]
            aa = np.minimum(1.0, 2.0 * a_)
            mu_l, mu_u = beta * self.mu * gamma, gamma * self.mu / beta
            par = np.ascontiguousarray(np.stack([aa, mu_l, mu_u], axis=1))
            tout = np.zeros((B, 2))
            self._call(self.L.tlpk_ipm_batch_targets(self.kkt._h, self._mask(cor), _lib.as_pd(par), _lib.as_pd(tout)))
            svl, svu = tout[:, 0], tout[:, 1]
            vt = (self.tau + aa * dtau) * (self.kappa + aa * dkappa)
            vt = np.where(vt < mu_l, mu_l - vt, np.where(vt > mu_u, mu_u - vt, 0.0))
            delta = (svl + svu + vt) / (self.p + 1)
            ctau, ckappa, av = self._newton(2, cor, 0.0, vt - delta, delta=delta)
            ctau = ctau + dtau; ckappa = ckappa + dkappa
            ac = self._max_step(av, ctau, ckappa)
            take = cor & (ac > a_)
            if take.any():
                self._call(self.L.tlpk_ipm_batch_accept(self.kkt._h, self._mask(take)))
                dtau = np.where(take, ctau, dtau); dkappa = np.where(take, ckappa, dkappa); alpha = np.where(take, ac, alpha)
            cor = cor & ~(ac < 1.1 * a_) & (ncor < o["CorrectionLimit"]) & (alpha < 0.999)      # an LP that breaks out is masked for the rest of the step
        alpha = alpha * o["StepDampFactor"]
        xz = np.zeros(B)
        self._call(self.L.tlpk_ipm_batch_advance(self.kkt._h, self._mask(step), _lib.as_pd(np.ascontiguousarray(alpha)), _lib.as_pd(xz)))
        self._set(self.tau, step, self.tau + alpha * dtau)
        self._set(self.kappa, step, self.kappa + alpha * dkappa)
        self._set(self.mu, step, (xz + self.tau * self.kappa) / (self.p + 1))
        return step

    # HSD.jl:203-350
    def optimize(self):
        if not self.loaded:
            raise RuntimeError("BatchedDeviceHSD(load=False): nothing is loaded on the device")
        tstart = time.perf_counter()
        self._call(self.L.tlpk_ipm_reset(self.kkt._h))
        self._init_state()
        act = self.active
        act[:] = True
        with np.errstate(all="ignore"):
            while act.any():
                self.compute_residuals(act)
                self.update_solver_status(act)
                act &= ~np.isin(self.status, _DECIDED)
                lim = act & (self.niter >= self._o["IterationsLimit"])
                self.status[lim] = "Trm_IterationLimit"
                act &= ~lim
                if not act.any():
                    break
                if time.perf_counter() - tstart >= self.time_limit:
                    self.status[act] = "Trm_TimeLimit"; act[:] = False; break
                try:
                    moved = self.compute_step(act)
                except OutOfMemoryError:
                    self.status[act] = "Trm_MemoryLimit"; act[:] = False; break
                act &= moved                                                 # (Trm_NumericalProblem: parked)
                self.niter[act] += 1
        self._cache = {}
        self.seconds = time.perf_counter() - tstart
        return self

    def _vec(self, what):
        if what not in self._cache:
            v = np.empty(self.m if what in _lib.IPM_GET_ROWS else self.n)
            self._call(self.L.tlpk_ipm_get(self.kkt._h, what, _lib.as_pd(v), v.shape[0]))
            self._cache[what] = v
        return self._cache[what]

    def _get(self, k, what):
        """Vector `what` (a code of tlpk_ipm_get: 0 x, 1 xl, 2 xu, 3 zl, 4 zu, 5 y, ... _lib.IPM_REGD) of LP k, as the device holds it."""
        off = self.row_off if what in _lib.IPM_GET_ROWS else self.col_off
        return self._vec(what)[off[k]:off[k + 1]].copy()

    def solution(self, k, nvar=None):
        """What `DeviceHSD.solution` returns, for LP k."""
        ray = "Sln_InfeasibilityCertificate" in (self.primal_status[k], self.dual_status[k])
        t_ = 1.0 if ray else 1.0 / self.tau[k]
        nk = int(self.col_off[k + 1] - self.col_off[k])
        n = nk if nvar is None else nvar
        x = self._get(k, 0)[:n] * t_
        s = (self._get(k, 3)[:n] - self._get(k, 4)[:n]) * t_
        y = self._get(k, 5) * t_
        sgn = 1.0 if self.objsense[k] else -1.0
        return {"status": str(self.status[k]), "niter": int(self.niter[k]), "x": x, "y": y, "s": s,
                "z_primal": sgn * float(self.primal_objective[k]), "z_dual": sgn * float(self.dual_objective[k]),
                "primal_status": str(self.primal_status[k]), "dual_status": str(self.dual_status[k]), "rho": tuple(float(v) for v in self.rho[k])}
