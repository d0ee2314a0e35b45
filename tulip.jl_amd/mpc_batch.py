"""Many small LPs in one set of launches through Mehrotra's predictor-corrector: the loop of mpc_device.py on a STACK of LPs
(DESIGN.md section 4b'').

`BatchedDeviceMPC` is to `BatchedDeviceHSD` what `DeviceMPC` is to `DeviceHSD`: the constructor, the stacking, the per-LP norms, the
residual call, the per-LP factor / retry loop with parking, `reload`, `_get` and `timers_of` are shared; tau = 1 and kappa = 0 throughout.
Every scalar of `DeviceMPC.optimize` / `compute_step` is a numpy array of length B and every branch a mask; the vector work goes through
the `tlpk_mpc_batch_*` calls (include/tlpk.h) and the shared `tlpk_ipm_batch_*` ones.  With B = 1 the run is `DeviceMPC`'s bit for bit.

    opt = BatchedDeviceMPC([standard_form(lp) for lp in lps], device=0).optimize()
    opt.status[k], opt.niter[k], opt.primal_objective[k], opt.solution(k)
"""
import time

import numpy as np

from . import _lib
from .hsd_batch import _DECIDED, BatchedDeviceHSD
from .hsd_device import SQRT_EPS
from .kkt import OutOfMemoryError


def _cube(r):
    """r ** 3 through Python's float power, as mpc_device.py computes it (numpy's power need not be libm's)."""
    try:
        return r ** 3
    except OverflowError:
        return float("inf")


class BatchedDeviceMPC(BatchedDeviceHSD):
    _bumped = ("regD", "regP")

    def _init_state(self):
        super()._init_state()                                                # tau = 1, regP = regD = 1 (MPC.jl:73-74)
        self.kappa = np.zeros(self.nlp)
        self.alpha_p, self.alpha_d = np.zeros(self.nlp), np.zeros(self.nlp)

    def _per_p(self, v):
        """v / p per LP, 0 for an LP without a finite bound (point.jl:45-48 without the tau-kappa term)."""
        return np.where(self.p > 0, v / np.where(self.p > 0, self.p, 1), 0.0)

    # MPC.jl:101-141: the HSD residual kernels with tau = 1
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
        self._set(self.primal_objective, act, self.cx + self.c0)
        self._set(self.dual_objective, act, self.dualsum + self.c0)
        self._set(self.mu, act, self._per_p(self.xz))

    # MPC.jl:149-214
    def update_solver_status(self, act):
        o = self._o
        rho_p = np.maximum(np.maximum(self.rp_nrm / (1 + self.nb), self.rl_nrm / (1 + self.nlz)), self.ru_nrm / (1 + self.nuz))
        rho_d = self.rd_nrm / (1 + self.nc)
        rho_g = np.abs(self.primal_objective - self.dual_objective) / (1 + np.abs(self.primal_objective))
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

    def compute_starting_point(self):                                        # MPC.jl:353-410, every LP
        out = np.zeros(self.nlp)
        self._call(self.L.tlpk_mpc_batch_start(self.kkt._h, _lib.as_pd(out)))
        self.timers["n_update"] += 1
        self.timers["n_solve"] += 2
        self.mu = self._per_p(out)

    def _newton(self, mode, m, gmu=0.0):
        """MPC/step.jl:164-217 for the LPs of `m`; returns the primal and dual step lengths (at most 1) as arrays."""
        g = np.ascontiguousarray(np.broadcast_to(np.asarray(gmu, dtype=np.float64), (self.nlp,)))
        out = np.zeros((self.nlp, 2))
        self._call(self.L.tlpk_mpc_batch_newton(self.kkt._h, mode, self._mask(m), _lib.as_pd(g), _lib.as_pd(out)))
        self.timers["n_solve"][m] += 1
        return np.minimum(1.0, out[:, 0]), np.minimum(1.0, out[:, 1])

    def _gap(self, m, ap, ad):
        out = np.zeros((self.nlp, 2))
        self._call(self.L.tlpk_mpc_batch_gap(self.kkt._h, self._mask(m), _lib.as_pd(np.ascontiguousarray(ap)), _lib.as_pd(np.ascontiguousarray(ad)),
                                             _lib.as_pd(out)))
        return out[:, 0].copy(), out[:, 1].copy()

    # MPC/step.jl:10-123 for the LPs of `act`; an LP that runs into the three-bump rule gets Trm_NumericalProblem and is parked
    def compute_step(self, act):
        step = act.copy()
        self._set(self.regP, step, np.minimum(np.maximum(self.regP / 10, SQRT_EPS), 1.0))      # step.jl:29-32 (uniform within an LP)
        self._set(self.regD, step, np.minimum(np.maximum(self.regD / 10, SQRT_EPS), 1.0))
        step = self._factor(step)
        if not step.any():
            return step
        with np.errstate(all="ignore"):
            return self._direction_and_move(step)

    def _direction_and_move(self, step):
        o = self._o
        # predictor (affine scaling), step.jl:225-241
        ap, ad = self._newton(0, step)
        # corrector, step.jl:246-274
        ga, _ = self._gap(step, ap, ad)
        ratio = (ga / self.p) / self.mu
        sigma = np.minimum(np.maximum(np.array([_cube(r) for r in ratio.tolist()]), SQRT_EPS), 1.0 - SQRT_EPS)
        ap, ad = self._newton(1, step, sigma * self.mu)
        # extra centrality corrections, step.jl:71-109, 279-322 (delta = 0.3, gamma = 0.1): while ANY LP still corrects
        ncor = np.zeros(self.nlp, dtype=np.int64)
        cor = step & (ncor < o["CorrectionLimit"])
        while cor.any():
            ap_, ad_ = np.minimum(ap + 0.3, 1.0), np.minimum(ad + 0.3, 1.0)
            ga, g = self._gap(cor, ap, ad)
            mu = (ga / g) * (ga / g) * (ga / self.p)
            par = np.ascontiguousarray(np.stack([ap_, ad_, mu * 0.1, mu / 0.1], axis=1))
            self._call(self.L.tlpk_mpc_batch_targets(self.kkt._h, self._mask(cor), _lib.as_pd(par)))
            apc, adc = self._newton(2, cor)
            take = cor & (apc >= 1.01 * ap) & (adc >= 1.01 * ad)
            if take.any():
                self._call(self.L.tlpk_ipm_batch_accept(self.kkt._h, self._mask(take)))
                ap, ad = np.where(take, apc, ap), np.where(take, adc, ad)
                ncor[take] += 1
            cor = take & (ncor < o["CorrectionLimit"])                       # a refused candidate or the limit: masked for the rest of the step
        ap, ad = ap * o["StepDampFactor"], ad * o["StepDampFactor"]
        self._set(self.alpha_p, step, ap); self._set(self.alpha_d, step, ad)
        xz = np.zeros(self.nlp)
        self._call(self.L.tlpk_mpc_batch_advance(self.kkt._h, self._mask(step), _lib.as_pd(np.ascontiguousarray(ap)), _lib.as_pd(np.ascontiguousarray(ad)),
                                                 _lib.as_pd(xz)))
        self._set(self.mu, step, self._per_p(xz))
        return step

    # MPC.jl:218-351
    def optimize(self):
        if not self.loaded:
            raise RuntimeError("BatchedDeviceMPC(load=False): nothing is loaded on the device")
        tstart = time.perf_counter()
        self._init_state()
        act = self.active
        act[:] = True
        with np.errstate(all="ignore"):
            self.compute_starting_point()
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


__all__ = ["BatchedDeviceMPC"]
