"""Many small LPs in one set of launches through Mehrotra's predictor-corrector: the loop of mpc_device.py on a STACK of LPs
(DESIGN.md section 4b'').

`BatchedDeviceMPC` is to `BatchedDeviceHSD` what `DeviceMPC` is to `DeviceHSD`: the constructor, the stacking, the per-LP norms, the
residual call, the per-LP factor / retry loop with parking, `reload`, `_get` and `timers_of` are shared; tau = 1 and kappa = 0 throughout.
Every scalar of `DeviceMPC.optimize` / `compute_step` is a numpy array of length B and every branch a mask; the vector work goes through
the `tlpk_mpc_batch_*` calls (include/tlpk.h) and the shared `tlpk_ipm_batch_*` ones.  With B = 1 the run is `DeviceMPC`'s bit for bit.

    opt = BatchedDeviceMPC([standard_form(lp) for lp in lps], device=0).optimize()
    opt.status[k], opt.niter[k], opt.primal_objective[k], opt.solution(k)

More LPs than slots (DESIGN.md section 4b''-s): `optimize_stream(queue)` as the HSD batch has it.  Mehrotra's starting point costs a factorisation and two
solves per LP; an LP that takes a slot pays for none of them: it is ENTERING for the rest of the pass in which its predecessor left -- the update of that
pass factorises its starting matrix beside the running LPs' iterates, the predictor solve and the corrector solve carry its two right-hand sides
(`tlpk_mpc_batch_factor_enter`, `tlpk_mpc_batch_newton_enter`) -- and `tlpk_mpc_batch_enter_finish` runs the column kernels of the starting point.

    pass p, after the leaves and the refill     active LPs                      entering LPs
      tlpk_mpc_batch_factor_enter               theta of the iterate, regP/regD   theta_inv = 0, Rp = 1, Rd = 1e-6
      tlpk_mpc_batch_newton_enter(0)            predictor                         (0, c) -> y
      tlpk_mpc_batch_newton_enter(1)            corrector                         (b, 0) -> x
      gap / targets / newton(2) / advance       as in optimize()                  skipped (their `active` flag is 0)
      tlpk_mpc_batch_enter_finish               --                                shifts, balanced products; active from pass p + 1
"""
import ctypes as C
import time

import numpy as np

from . import _lib
from .batch_retry import check_retry, factor_failed
from .hsd_batch import _DECIDED, BatchedDeviceHSD, stream_assign
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
        self.timers["n_update_calls"] += 1
        self.timers["n_lp_factor"] += self.nlp
        self.timers["n_solve"] += 2
        self.mu = self._per_p(out)

    def _newton(self, mode, m, gmu=0.0, enter=None):
        """MPC/step.jl:164-217 for the LPs of `m`; returns the primal and dual step lengths (at most 1) as arrays.
        enter (modes 0, 1): the LPs that take a solve of their starting point from the same stacked solve."""
        g = np.ascontiguousarray(np.broadcast_to(np.asarray(gmu, dtype=np.float64), (self.nlp,)))
        out = np.zeros((self.nlp, 2))
        if enter is not None and enter.any():
            e8 = np.ascontiguousarray(enter, dtype=np.uint8)
            self._call(self.L.tlpk_mpc_batch_newton_enter(self.kkt._h, mode, self._mask(m), _lib.as_pu8(e8), _lib.as_pd(g), _lib.as_pd(out)))
            self.timers["n_solve"][enter] += 1
        else:
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

    def _direction_and_move(self, step, enter=None):
        o = self._o
        # predictor (affine scaling), step.jl:225-241
        ap, ad = self._newton(0, step, enter=enter)
        # corrector, step.jl:246-274
        if step.any():
            ga, _ = self._gap(step, ap, ad)
            ratio = (ga / self.p) / self.mu
            sigma = np.minimum(np.maximum(np.array([_cube(r) for r in ratio.tolist()]), SQRT_EPS), 1.0 - SQRT_EPS)
        else:
            sigma = np.zeros(self.nlp)                                       # (a pass in which only entering LPs are left: their second solve)
        ap, ad = self._newton(1, step, sigma * self.mu, enter=enter)
        if not step.any():
            return step
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
            self.corrector_rounds += 1                                       # (a statistic: rounds of the centrality corrector, summed over the steps)
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

    # ---- a batch that keeps going (DESIGN.md section 4b''-s) ----
    def _init_slot(self, k):
        super()._init_slot(k)
        self.kappa[k] = 0.0
        self.alpha_p[k] = self.alpha_d[k] = 0.0

    def _factor_enter(self, step, enter):
        """`_factor` with entering LPs in the update: returns (the LPs of `step` that hold a factor, the LPs of `enter` whose starting matrix was factorised).
        An entering LP that the update names as its failure is out with Trm_NumericalProblem: its regularisations are the starting point's constants, there is
        nothing to bump.  The others retry as in `_factor`."""
        if not enter.any():
            return self._factor(step), enter.copy()
        if self.retry == "failed":
            return factor_failed(self, step, enter, self._factor_each)
        B = self.nlp
        step, enter, entering = step.copy(), enter.copy(), enter.copy()
        nbump = np.zeros(B, dtype=np.int64)
        fail = C.c_int64(-1)
        while step.any() or enter.any():
            s8, e8 = np.ascontiguousarray(step, dtype=np.uint8), np.ascontiguousarray(enter, dtype=np.uint8)
            rc = self.L.tlpk_mpc_batch_factor_enter(self.kkt._h, _lib.as_pu8(s8), _lib.as_pu8(e8), _lib.as_pd(self.regP), _lib.as_pd(self.regD), C.byref(fail))
            self.last_update_rc = rc
            self.timers["n_update_calls"] += 1
            self.timers["n_lp_factor"] += int((step | enter).sum())
            if rc == _lib.OK:
                self.timers["n_update"][step | enter] += 1
                break
            if rc != _lib.NOT_POSDEF:
                self._call(rc)
            k = int(fail.value)
            if 0 <= k < B and enter[k]:
                self.status[k] = "Trm_NumericalProblem"
                enter[k] = False
                self._evict(k)
                continue
            bad = np.zeros(B, dtype=bool)
            if 0 <= k < B and step[k]:
                bad[k] = True
            else:
                bad[:] = step | enter                                        # the pivot cannot be attributed: every LP of the update counts a failure
            for name in self._bumped:
                getattr(self, name)[bad & step] *= 100
            nbump[bad] += 1
            self.timers["n_bump"][bad & step] += 1
            gone = bad & ~(nbump < 3)
            self.status[gone] = "Trm_NumericalProblem"
            step &= ~gone; enter &= ~gone
        self.timers["max_bumps_in_a_step"] = np.maximum(self.timers["max_bumps_in_a_step"], np.where(entering, 0, nbump))
        if nbump.any():
            self.bump_log.append(nbump.copy())
        return step, enter

    def _evict(self, k):
        """The starting matrix of the LP in slot k was refused.  From here on the slot is parked, and a parked block is factorised with every update unless
        `skip_parked` leaves it out: values that broke the starting matrix (an entry that is not a number, say) would break the parked one as well and fail
        the updates of every other LP.  So the slot takes back the matrix values of the LP it replaced, which this slot has factorised before; its vectors
        and the record of the refused LP stay (its iterate is the one `_apply` left: the update failed before anything was written)."""
        old = self._replaced.pop(k, None)
        if old is None:
            return
        p0, p1 = self._slot_range(k)
        self.A.data[p0:p1] = old
        sel = np.zeros(self.nlp, dtype=np.uint8); sel[k] = 1
        nz = self.A.data
        t0 = time.perf_counter()
        self._call(self.L.tlpk_ipm_batch_refill(self.kkt._h, _lib.as_pu8(sel), _lib.as_pd(nz), nz.shape[0], None, None, None, None))
        self.refill_seconds += time.perf_counter() - t0

    def _enter_finish(self, enter):
        out = np.zeros(self.nlp)
        t0 = time.perf_counter()
        e8 = np.ascontiguousarray(enter, dtype=np.uint8)
        self._call(self.L.tlpk_mpc_batch_enter_finish(self.kkt._h, _lib.as_pu8(e8), _lib.as_pd(out)))
        self.enter_finish_seconds += time.perf_counter() - t0
        self._set(self.mu, enter, self._per_p(out))

    enter_finish_seconds = 0.0

    def _step_stream(self, act, enter):
        """`compute_step` for the LPs of `act` with the LPs of `enter` riding along; returns (the active LPs that moved, the entering LPs that now stand at
        their starting point)."""
        step = act.copy()
        self._set(self.regP, step, np.minimum(np.maximum(self.regP / 10, SQRT_EPS), 1.0))
        self._set(self.regD, step, np.minimum(np.maximum(self.regD / 10, SQRT_EPS), 1.0))
        step, enter = self._factor_enter(step, enter)
        if step.any() or enter.any():                                        # the two entering solves happen also when no active LP holds a factor
            self._direction_and_move(step, enter)
        if enter.any():
            self._enter_finish(enter)
        return step, enter

    def refill(self, slots, lps, options=None, retry=None):
        """`BatchedDeviceHSD.refill`, then Mehrotra's starting point for those slots alone (no LP is active in the four calls, the new ones enter).  An LP
        whose starting matrix cannot be factorised ends Trm_NumericalProblem."""
        super().refill(slots, lps, options, retry=retry)
        enter = np.zeros(self.nlp, dtype=bool)
        enter[[int(k) for k in slots]] = True
        with np.errstate(all="ignore"):
            self._step_stream(np.zeros(self.nlp, dtype=bool), enter)
        return self

    def optimize_stream(self, lps, options=None, retry=None):
        """`BatchedDeviceHSD.optimize_stream` for Mehrotra's loop: the same records, the same FIFO schedule (`stream_assign`), options that travel with the LP,
        `passes`, `refills`, `refill_seconds`, `record_seconds` (and `enter_finish_seconds`).  An LP found decided in pass p leaves in pass p; its slot is
        refilled straight after the leaves of that pass and the new LP is ENTERING for the rest of it (module docstring), active from pass p + 1 -- the pass its
        record names as `entered`.  A slot so holds an LP for niter + 1 passes.  An entering LP whose starting matrix fails the update gets
        Trm_NumericalProblem with niter 0 (entered = left = p) and frees its slot."""
        B = self.nlp
        if retry is not None:
            self.retry = check_retry(retry)
        queue, qopts, slot_keys, qkeys = self._stream_queue(lps, options)
        N = len(queue)
        tstart = time.perf_counter()
        time_limit = min([self.time_limit] + [float(o.TimeLimit) for o in qopts])
        self._init_state()
        act = self.active
        act[:] = True
        enter = np.zeros(B, dtype=bool)
        records = [None] * (B + N)
        lp_of_slot, entered, free, waiting = list(range(B)), [1] * B, set(), list(range(N))
        self.passes = self.refills = 0
        self.refill_seconds = self.record_seconds = self.enter_finish_seconds = 0.0
        self.corrector_rounds = 0
        stopped = None

        def leave(mask):
            self._leave(mask, records, lp_of_slot, entered, free)

        def assign():
            return stream_assign(free, slot_keys, [qkeys[q] for q in waiting]) if free and waiting else []

        with np.errstate(all="ignore"):
            self.compute_starting_point()
            while act.any() or assign():
                self.passes += 1
                before = act.copy()
                if act.any():
                    self.compute_residuals(act)
                    self.update_solver_status(act)
                    act &= ~np.isin(self.status, _DECIDED)
                    lim = act & (self.niter >= self._o["IterationsLimit"])
                    self.status[lim] = "Trm_IterationLimit"
                    act &= ~lim
                    leave(before & ~act)
                pairs = assign()                                             # straight after the leaves: the new LPs enter in this pass
                if pairs:
                    qs = [waiting[pos] for _, pos in pairs]
                    self._apply([(k,) + queue[q][1:] for (k, _), q in zip(pairs, qs)], [qopts[q] for q in qs])
                    for (k, _), q in zip(pairs, qs):
                        lp_of_slot[k], entered[k] = B + q, self.passes + 1
                        free.discard(k); enter[k] = True
                    gone = set(qs)
                    waiting = [q for q in waiting if q not in gone]
                if not (act.any() or enter.any()):
                    break
                if time.perf_counter() - tstart >= time_limit:
                    self.status[act | enter] = stopped = "Trm_TimeLimit"; leave(act | enter); act[:] = False; break
                try:
                    moved, entered_now = self._step_stream(act, enter)
                except OutOfMemoryError:
                    self.status[act | enter] = stopped = "Trm_MemoryLimit"; leave(act | enter); act[:] = False; break
                failed = act & ~moved                                        # (Trm_NumericalProblem: the slot is free like any other)
                failed_entering = enter & ~entered_now
                for k in np.flatnonzero(failed_entering):
                    entered[k] = self.passes                                 # (it never became active)
                act &= moved
                leave(failed | failed_entering)
                self.niter[act] += 1
                act |= entered_now                                           # active from the next pass
                enter[:] = False
        for q in waiting:                                                    # (only after a global stop: these LPs never ran)
            records[B + q] = self._never_ran(queue[q], stopped)
        self._cache = {}
        self.seconds = time.perf_counter() - tstart
        self.records = records
        return records


__all__ = ["BatchedDeviceMPC"]
