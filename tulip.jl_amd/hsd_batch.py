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

More LPs than slots (DESIGN.md section 4b'-r): the B LPs of the constructor are the first occupants of B slots, a queue streams through them --
a slot whose LP is decided takes the next LP of its pattern (`refill`: tlpk_ipm_batch_refill) while the others continue.

    records = opt.optimize_stream(more_lps)      # one record per LP of constructor + queue; opt.passes
"""
import ctypes as C
import time

import numpy as np

from . import _lib
from .batch_retry import check_retry, factor_failed, warn_hold_refused
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


def _csc(A):
    """A as a canonical scipy CSC matrix (sorted row indices, duplicates summed); the caller's matrix is not modified."""
    import scipy.sparse as sp
    A = sp.csc_matrix(A, dtype=np.float64, copy=True) if sp.issparse(A) else sp.csc_matrix(np.asarray(A, dtype=np.float64))
    A.sum_duplicates()
    return A


def pattern_key(A):
    """What two LPs must share to take turns in one slot of an analysed handle: the shape, the column pointers and the row indices of A
    (stored entries count, their values do not).  Equal patterns give equal keys; a moved entry or another shape gives another key."""
    return _key(_csc(A))


def _key(A):
    return (tuple(int(v) for v in A.shape), A.indptr.astype(np.int64).tobytes(), A.indices.astype(np.int64).tobytes())


def stream_assign(free_slots, slot_keys, queue_keys):
    """The schedule of `optimize_stream` at the top of one pass: every free slot, in slot order, takes the FIRST LP of the queue whose pattern
    is the slot's.  free_slots: slot numbers; slot_keys[k]: the pattern key of slot k; queue_keys: the keys of the LPs still waiting, in
    queue order.  Returns [(slot, position in the queue)]; a slot with no matching LP left is not in the list (it stays parked)."""
    taken, out = set(), []
    for k in sorted(free_slots):
        for pos, key in enumerate(queue_keys):
            if pos not in taken and key == slot_keys[k]:
                taken.add(pos); out.append((k, pos))
                break
    return out


class BatchedDeviceHSD:
    def __init__(self, lps, system="K1", options=None, load=True, skip_parked=False, retry="all", **backend_kw):
        # options: one Options for every LP, or a sequence with one per LP
        # skip_parked=True: the blocks of the LPs a call's mask leaves out are skipped inside the factorisation and the sweeps (tlpk_ipm_batch_skip); the results
        # of optimize() / optimize_stream() do not depend on it, bit for bit.  Silently off on handles with refine > 0 (the refinement's norms run over all rows).
        # Off by default: with it on, an LP that a tlpk_ipm_batch_factor call left out has NO factor of the parking values -- a caller that drives the
        # tlpk_ipm_batch_* calls itself and solves such an LP gets unspecified values where it used to get the solve against the parked block (the loops here
        # never do that; tests/test_ipm_kernels.py's call-by-call sequences do)
        # retry="all": an update that fails names one LP, which is bumped, and the whole stack is factorised again.  retry="failed": every LP that failed in
        # an update is named and bumped (tlpk_ipm_batch_factor_each), the next update factorises those alone and the others keep their factor
        # (batch_retry.py; DESIGN.md section 4b'-v).  Per LP the two settings give the same run, bit for bit; "failed" falls back to "all", with a warning,
        # where the library cannot hold a factor (refine > 0, or an ordering that mixes the LPs' fronts)
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
        self.retry = check_retry(retry)
        self._host_norms()
        self._init_state()
        self.last_update_rc = None
        self.passes = self.refills = 0                                           # optimize_stream: trips round the loop; refill calls, the time inside them and in reading records
        self.refill_seconds = self.record_seconds = 0.0
        self.corrector_rounds = 0
        self._replaced = {}                                                      # slot -> the matrix values of the LP its present one replaced (`_apply`)
        self.loaded = False
        if load:
            self._call(self.L.tlpk_ipm_load_batch(self.kkt._h, B, _lib.as_p64(self.row_off), _lib.as_p64(self.col_off),
                                                  _lib.as_pd(self._b), _lib.as_pd(self._c), _lib.as_pd(self._l), _lib.as_pd(self._u)))
            self.loaded = True
        self._can_skip = self.loaded and int(backend_kw.get("refine", 0)) == 0
        self.skip_parked = False
        self.set_skip_parked(skip_parked)

    def set_skip_parked(self, on):
        """Switch the skipping of parked blocks (tlpk_ipm_batch_skip) on or off between runs; stays off on a handle with refine > 0."""
        on = bool(on) and self._can_skip
        if on != self.skip_parked:
            self._call(self.L.tlpk_ipm_batch_skip(self.kkt._h, int(on)))
            self.skip_parked = on
        return self

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
        self.timers["n_update_calls"] = 0                                    # update calls of the BATCH in this run, under either `retry` (a number, not per LP)
        self.timers["n_lp_factor"] = 0                                       # ... and the LPs they were asked to factorise, summed over the calls
        self.bump_log = []                                                   # per pass in which an update failed: how often each LP was bumped in it
        self.rho = np.zeros((B, 3))
        for name in ("rp_nrm", "rl_nrm", "ru_nrm", "rd_nrm", "cx", "xz", "ax_nrm", "xxl_nrm", "xxu_nrm", "delta_nrm", "dualsum", "rg_nrm",
                     "primal_objective", "dual_objective"):
            setattr(self, name, np.zeros(B))
        self.seconds = 0.0
        self._cache = {}

    def timers_of(self, k):
        """The timers of LP k as `DeviceHSD.timers` holds them."""
        return {name: int(v[k]) for name, v in self.timers.items() if isinstance(v, np.ndarray)}

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

    def _slot_range(self, k):
        """Where LP k's entries sit in the stacked matrix's value array (block-diagonal CSC: the columns of an LP are contiguous)."""
        return int(self.A.indptr[self.col_off[k]]), int(self.A.indptr[self.col_off[k + 1]])

    def slot_key(self, k):
        """`pattern_key` of the LP slot k was analysed with."""
        p0, p1 = self._slot_range(k)
        indptr = self.A.indptr[self.col_off[k]:self.col_off[k + 1] + 1].astype(np.int64) - p0
        indices = self.A.indices[p0:p1].astype(np.int64) - self.row_off[k]
        shape = (int(self.row_off[k + 1] - self.row_off[k]), int(self.col_off[k + 1] - self.col_off[k]))
        return (shape, indptr.tobytes(), indices.tobytes())

    def _hsd_only(self, what):
        # a subclass that brings its own loop brings its own stream (BatchedDeviceMPC does: the starting point of an LP that enters a slot, a factorisation
        # and two solves, rides in the update and the solves of the running LPs); one that does not cannot borrow this one
        if type(self).optimize is not BatchedDeviceHSD.optimize and type(self).optimize_stream is BatchedDeviceHSD.optimize_stream:
            raise NotImplementedError(f"{what} serves the homogeneous self-dual loop only: {type(self).__name__} has no refill")

    def _per_lp(self, options, count, what):
        if options is None or isinstance(options, Options) or isinstance(options, type):
            return [options or Options()] * count
        options = list(options)
        if len(options) != count:
            raise ValueError(f"{what}: one Options object, or one per LP")
        return options

    def refill(self, slots, lps, options=None, retry=None):
        """New LPs for the listed slots of the analysed handle (tlpk_ipm_batch_refill): lps[i] replaces the LP of slots[i] -- matrix values, b, c, l,
        u, c0, objective sense, options (default: `Options()`) -- and starts from the HSD starting point with its host state (tau, kappa, mu,
        regularisations, niter, statuses, timers, recorded norms) re-initialised; every other slot continues untouched.  An LP whose pattern
        (shape, column pointers, row indices) differs from its slot's raises ValueError, and nothing is changed."""
        self._hsd_only("refill")
        if retry is not None:                                                # (how the updates after the refill retry: the constructor's `retry`)
            self.retry = check_retry(retry)
        slots = [int(k) for k in slots]
        lps = list(lps)
        if len(slots) != len(lps) or len(set(slots)) != len(slots) or any(not 0 <= k < self.nlp for k in slots):
            raise ValueError("refill: one LP per listed slot, every slot listed once, slots in 0 .. nlp - 1")
        opts = self._per_lp(options, len(slots), "refill options")
        staged = []
        for k, lp in zip(slots, lps):
            st = self._stage(lp, f"refill, slot {k}")
            if st[0] != self.slot_key(k):
                raise ValueError(f"refill: the pattern of the LP for slot {k} (shape, column pointers, row indices) differs from the slot's")
            staged.append((k,) + st[1:])
        if not self.loaded:
            raise RuntimeError("BatchedDeviceHSD(load=False): nothing is loaded on the device")
        return self._apply(staged, opts)

    @staticmethod
    def _stage(lp, where, memo=None):
        """(pattern key, values in canonical CSC order, [b, c, l, u], c0, objsense) of one LP that is to enter a slot; the vectors are checked against A.
        memo: LPs that share one matrix OBJECT (the same A under many costs) share its canonical copy and its key."""
        A, b, c, l, u, c0, sense = _fields(lp)
        if memo is not None and id(A) in memo:
            A, key = memo[id(A)][1:]
        else:
            A0, A = A, _csc(A)
            key = _key(A)
            if memo is not None:
                memo[id(A0)] = (A0, A, key)                                  # (holds A0: its id stays its own for the memo's lifetime)
        mk, nk = A.shape
        vecs = []
        for v, length, what in ((b, mk, "b"), (c, nk, "c"), (l, nk, "l"), (u, nk, "u")):
            a = np.asarray(v, dtype=np.float64)
            if a.shape != (length,):
                raise DimensionMismatch(f"{where}: {what} does not match A")
            vecs.append(a)
        return key, A.data, vecs, c0, sense

    def _apply(self, staged, opts):
        """`refill` behind its checks: staged = [(slot, values, [b, c, l, u], c0, objsense)] with the slots' own patterns."""
        if not staged:
            return self
        sel = np.zeros(self.nlp, dtype=np.uint8)
        # an array in which no selected LP changes a bit (the same matrix under new costs, the same bounds) is not sent: NULL = keep
        same = lambda dst, src: np.array_equal(dst.view(np.int64), np.ascontiguousarray(src).view(np.int64))      # noqa: E731
        new = dict.fromkeys(("A", "b", "c", "l", "u"), False)
        for (k, data, vecs, c0, sense), o in zip(staged, opts):
            p0, p1 = self._slot_range(k)
            rs, cs = slice(self.row_off[k], self.row_off[k + 1]), slice(self.col_off[k], self.col_off[k + 1])
            for name, dst, src in (("A", self.A.data[p0:p1], data), ("b", self._b[rs], vecs[0]), ("c", self._c[cs], vecs[1]),
                                   ("l", self._l[cs], vecs[2]), ("u", self._u[cs], vecs[3])):
                if not same(dst, src):
                    new[name] = True
                    if name == "A":
                        self._replaced[k] = dst.copy()
                    dst[:] = src
            self.c0[k] = c0; self.objsense[k] = sense
            sel[k] = 1
        nz = self.A.data
        ptr = lambda name, a: _lib.as_pd(a) if new[name] else None           # noqa: E731
        t0 = time.perf_counter()
        self._call(self.L.tlpk_ipm_batch_refill(self.kkt._h, _lib.as_pu8(sel), ptr("A", nz), nz.shape[0],
                                                ptr("b", self._b), ptr("c", self._c), ptr("l", self._l), ptr("u", self._u)))
        self.refills += 1; self.refill_seconds += time.perf_counter() - t0     # (the call returns when the device has finished)
        self.opts = list(self.opts)
        for (k, *_rest), o in zip(staged, opts):
            self._host_norms_of(k)
            self._init_slot(k)
            self.opts[k] = o
            for name, arr in self._o.items():
                arr[k] = float(getattr(o, name))
            self.time_limit = min(self.time_limit, float(o.TimeLimit))
        self._cache = {}
        return self

    def _host_norms_of(self, k):
        """`_host_norms` for slot k alone."""
        rs, cs = slice(self.row_off[k], self.row_off[k + 1]), slice(self.col_off[k], self.col_off[k + 1])
        l, u = self._l[cs], self._u[cs]
        lf, uf = np.isfinite(l), np.isfinite(u)
        nrm = lambda v: float(np.abs(v).max(initial=0.0))                    # noqa: E731
        self.p[k] = int(lf.sum()) + int(uf.sum())
        self.nb[k], self.nc[k] = nrm(self._b[rs]), nrm(self._c[cs])
        self.nlz[k], self.nuz[k] = nrm(np.where(lf, l, 0.0)), nrm(np.where(uf, u, 0.0))

    def _init_slot(self, k):
        """`_init_state` for slot k alone."""
        for v in (self.regP, self.regD, self.regG, self.tau, self.kappa, self.mu):
            v[k] = 1.0
        self.rg[k] = self.h0[k] = 0.0
        self.niter[k] = 0
        self.status[k] = "Trm_Unknown"; self.primal_status[k] = "Sln_Unknown"; self.dual_status[k] = "Sln_Unknown"
        self.active[k] = False
        for v in self.timers.values():
            if isinstance(v, np.ndarray):
                v[k] = 0
        self.rho[k] = 0.0
        for name in ("rp_nrm", "rl_nrm", "ru_nrm", "rd_nrm", "cx", "xz", "ax_nrm", "xxl_nrm", "xxu_nrm", "delta_nrm", "dualsum", "rg_nrm",
                     "primal_objective", "dual_objective"):
            getattr(self, name)[k] = 0.0

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
        if self.retry == "failed":
            return factor_failed(self, step, np.zeros(self.nlp, dtype=bool), self._factor_each)[0]
        B = self.nlp
        step = step.copy()
        nbump = np.zeros(B, dtype=np.int64)
        fail = C.c_int64(-1)
        while step.any():                                                    # step.jl:35-51, per LP
            rc = self.L.tlpk_ipm_batch_factor(self.kkt._h, self._mask(step), _lib.as_pd(self.regP), _lib.as_pd(self.regD), C.byref(fail))
            self.last_update_rc = rc
            self.timers["n_update_calls"] += 1
            self.timers["n_lp_factor"] += int(step.sum())
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
        if nbump.any():
            self.bump_log.append(nbump.copy())
        return step

    def _factor_each(self, role):
        """One tlpk_ipm_batch_factor_each with the roles of batch_retry.factor_failed: (rc, fail_col)."""
        role = np.ascontiguousarray(role, dtype=np.uint8)
        fail_col = np.full(self.nlp, -1, dtype=np.int64)
        nfail = C.c_int64(0)
        rc = self.L.tlpk_ipm_batch_factor_each(self.kkt._h, _lib.as_pu8(role), _lib.as_pd(self.regP), _lib.as_pd(self.regD), _lib.as_p64(fail_col), C.byref(nfail))
        return rc, fail_col

    def _last_error(self):
        return self.L.tlpk_last_error(self.kkt._h).decode()

    def _hold_refused(self):
        """The library refused a hold (batch_retry.factor_failed): this object retries with whole updates from here on, and says so once."""
        if self.retry == "failed":
            self.retry = "all"
            warn_hold_refused(self, self._last_error())

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
        self.corrector_rounds += ncor                                        # (a statistic: rounds of the centrality corrector, summed over the steps)
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

    # ---- a batch that keeps going (DESIGN.md section 4b'-r) ----
    def optimize_stream(self, lps, options=None, retry=None):
        """N LPs through the B slots of this handle: the LPs of the constructor are the first occupants, `lps` is the queue.  When an LP leaves
        (decided, iteration limit, numerical problem) its record is read through tlpk_ipm_get_lps and, at the top of the next pass, its slot takes
        the first LP of the queue whose pattern is the slot's (`stream_assign`; `refill`) while every other slot continues untouched.  The
        schedule is deterministic.  options: for the LPs of the queue (one `Options`, or one per LP; default `Options()`) -- options travel
        with the LP, not with the slot.  IterationsLimit counts per LP, TimeLimit is global.  One pass is one trip round the loop of
        `optimize()`; `self.passes` counts them.  Returns one record per LP of constructor + queue, in that order: what `solution(k)`
        returns, plus zl, zu and the homogeneous iterate xh, yh as the device holds them, tau, timers, the slot the LP ran in and the
        passes (1-based) in which it entered and left.  A queue LP that matches no slot raises ValueError before anything runs."""
        self._hsd_only("optimize_stream")
        if retry is not None:                                                # (the constructor's `retry`, for this run and the following ones)
            self.retry = check_retry(retry)
        B = self.nlp
        queue, qopts, slot_keys, qkeys = self._stream_queue(lps, options)
        N = len(queue)
        tstart = time.perf_counter()
        time_limit = min([self.time_limit] + [float(o.TimeLimit) for o in qopts])
        self._call(self.L.tlpk_ipm_reset(self.kkt._h))
        self._init_state()
        act = self.active
        act[:] = True
        records = [None] * (B + N)
        lp_of_slot, entered, free, waiting = list(range(B)), [1] * B, set(), list(range(N))
        self.passes = self.refills = 0
        self.refill_seconds = self.record_seconds = 0.0
        self.corrector_rounds = 0
        stopped = None

        def leave(mask):
            self._leave(mask, records, lp_of_slot, entered, free)

        with np.errstate(all="ignore"):
            while True:
                if free and waiting:
                    pairs = stream_assign(free, slot_keys, [qkeys[q] for q in waiting])
                    if pairs:
                        qs = [waiting[pos] for _, pos in pairs]
                        self._apply([(k,) + queue[q][1:] for (k, _), q in zip(pairs, qs)], [qopts[q] for q in qs])
                        for (k, _), q in zip(pairs, qs):
                            lp_of_slot[k], entered[k] = B + q, self.passes + 1
                            free.discard(k); act[k] = True
                        gone = set(qs)
                        waiting = [q for q in waiting if q not in gone]
                if not act.any():
                    break
                self.passes += 1
                before = act.copy()
                self.compute_residuals(act)
                self.update_solver_status(act)
                act &= ~np.isin(self.status, _DECIDED)
                lim = act & (self.niter >= self._o["IterationsLimit"])
                self.status[lim] = "Trm_IterationLimit"
                act &= ~lim
                leave(before & ~act)
                if not act.any():
                    continue
                if time.perf_counter() - tstart >= time_limit:
                    self.status[act] = stopped = "Trm_TimeLimit"; leave(act); act[:] = False; break
                try:
                    moved = self.compute_step(act)
                except OutOfMemoryError:
                    self.status[act] = stopped = "Trm_MemoryLimit"; leave(act); act[:] = False; break
                failed = act & ~moved                                        # (Trm_NumericalProblem: the slot is free like any other)
                act &= moved
                leave(failed)
                self.niter[act] += 1
        for q in waiting:                                                    # (only after a global stop: these LPs never ran)
            records[B + q] = self._never_ran(queue[q], stopped)
        self._cache = {}
        self.seconds = time.perf_counter() - tstart
        self.records = records
        return records

    def _stream_queue(self, lps, options):
        """What `optimize_stream` checks before anything runs: the queue staged (`_stage`), its options, and the pattern of every slot and every waiting LP
        as small integers (the schedule compares those)."""
        memo = {}
        queue = [self._stage(lp, f"optimize_stream, LP {q} of the queue", memo) for q, lp in enumerate(lps)]
        qopts = self._per_lp(options, len(queue), "optimize_stream options")
        number = {}
        slot_keys = [number.setdefault(self.slot_key(k), len(number)) for k in range(self.nlp)]
        qkeys = [number.get(st[0], -1) for st in queue]
        for q, key in enumerate(qkeys):
            if key < 0:
                raise ValueError(f"optimize_stream: LP {q} of the queue has the pattern (shape, column pointers, row indices) of no slot")
        if not self.loaded:
            raise RuntimeError(f"{type(self).__name__}(load=False): nothing is loaded on the device")
        return queue, qopts, slot_keys, qkeys

    @staticmethod
    def _never_ran(staged, stopped):
        zn, zm = np.zeros(len(staged[2][1])), np.zeros(len(staged[2][0]))
        return {"status": stopped, "niter": 0, "x": zn, "y": zm, "s": zn, "z_primal": 0.0, "z_dual": 0.0, "primal_status": "Sln_Unknown",
                "dual_status": "Sln_Unknown", "rho": (0.0, 0.0, 0.0), "zl": zn, "zu": zn, "xh": zn, "yh": zm, "tau": 1.0, "timers": {},
                "slot": None, "entered": None, "left": None, "primal_objective": 0.0, "dual_objective": 0.0}

    gather_records = True                                                    # the records of the LPs that leave in one pass: one tlpk_ipm_get_lps (False: four tlpk_ipm_get_lp per LP)

    def _leave(self, mask, records, lp_of_slot, entered, free):
        """The LPs of `mask` leave in this pass: their records are read, their slots are free."""
        ks = [int(k) for k in np.flatnonzero(mask)]
        if not ks:
            return
        t0 = time.perf_counter()
        vecs = self._get_lps(ks, (0, 3, 4, 5)) if self.gather_records else [None] * len(ks)
        for k, vec in zip(ks, vecs):
            records[lp_of_slot[k]] = self._record(k, entered[k], self.passes, vec)
            free.add(k)
        self.record_seconds += time.perf_counter() - t0

    def _get_lps(self, ks, codes):
        """[{code: segment}] for the LPs `ks` through ONE tlpk_ipm_get_lps: one gather kernel, one copy."""
        lens = [[int((self.row_off if what in _lib.IPM_GET_ROWS else self.col_off)[k + 1] - (self.row_off if what in _lib.IPM_GET_ROWS else self.col_off)[k])
                 for what in codes] for k in ks]
        buf = np.empty(sum(sum(row) for row in lens))
        what, lp = np.array(codes, dtype=np.int32), np.array(ks, dtype=np.int64)
        self._call(self.L.tlpk_ipm_get_lps(self.kkt._h, what.ctypes.data_as(C.POINTER(C.c_int32)), what.shape[0], _lib.as_p64(lp), lp.shape[0],
                                           _lib.as_pd(buf), buf.shape[0]))
        out, pos = [], 0
        for row in lens:
            vec = {}
            for what_, length in zip(codes, row):
                vec[what_] = buf[pos:pos + length].copy(); pos += length
            out.append(vec)
        return out

    def _get_lp(self, k, what):
        """`_get` through tlpk_ipm_get_lp: LP k's segment alone crosses the bus."""
        off = self.row_off if what in _lib.IPM_GET_ROWS else self.col_off
        v = np.empty(int(off[k + 1] - off[k]))
        self._call(self.L.tlpk_ipm_get_lp(self.kkt._h, what, k, _lib.as_pd(v), v.shape[0]))
        return v

    def _record(self, k, entered, left, vec=None):
        vec = vec or {what: self._get_lp(k, what) for what in (0, 3, 4, 5)}
        rec = self._solution(k, None, lambda _k, what: vec[what])
        rec.update(zl=vec[3], zu=vec[4], xh=vec[0], yh=vec[5], tau=float(self.tau[k]), timers=self.timers_of(k), slot=k, entered=entered, left=left,
                   primal_objective=float(self.primal_objective[k]), dual_objective=float(self.dual_objective[k]))
        return rec

    def solution(self, k, nvar=None):
        """What `DeviceHSD.solution` returns, for LP k."""
        return self._solution(k, nvar, self._get)

    def _solution(self, k, nvar, get):
        ray = "Sln_InfeasibilityCertificate" in (self.primal_status[k], self.dual_status[k])
        t_ = 1.0 if ray else 1.0 / self.tau[k]
        nk = int(self.col_off[k + 1] - self.col_off[k])
        n = nk if nvar is None else nvar
        x = get(k, 0)[:n] * t_
        s = (get(k, 3)[:n] - get(k, 4)[:n]) * t_
        y = get(k, 5) * t_
        sgn = 1.0 if self.objsense[k] else -1.0
        return {"status": str(self.status[k]), "niter": int(self.niter[k]), "x": x, "y": y, "s": s,
                "z_primal": sgn * float(self.primal_objective[k]), "z_dual": sgn * float(self.dual_objective[k]),
                "primal_status": str(self.primal_status[k]), "dual_status": str(self.dual_status[k]), "rho": tuple(float(v) for v in self.rho[k])}
