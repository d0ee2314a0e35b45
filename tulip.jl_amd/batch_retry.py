"""The retry loop of a batched update with a verdict per LP (`tlpk_ipm_batch_factor_each`; DESIGN.md section 4b'-v), shared by
`BatchedDeviceHSD` and `BatchedDeviceMPC` under `retry="failed"`.

`retry="all"` (the default, hsd_batch.py `_factor` / mpc_batch.py `_factor_enter`) learns of ONE failing LP per update and factorises the whole
stack again after every bump: K LPs that fail in one pass cost at least K + 1 updates of all B blocks.  Here every LP that failed is bumped in the
same round, the next call factorises only those, and the LPs that came through keep their factor (role 2, hold).  An LP's regularisations, its
bump count, its status and the values its factor is made of are the same under both settings: the LPs of a stack do not see each other.

The loop takes the update as a callable, so it runs without a device (tests/test_batch_retry.py drives it with a stub)."""
import warnings

import numpy as np

from . import _lib

RETRY_MODES = ("all", "failed")
ROLE_PARKED, ROLE_ACTIVE, ROLE_HOLD, ROLE_ENTERING = 0, 1, 2, 3


def check_retry(retry):
    if retry not in RETRY_MODES:
        raise ValueError(f"retry must be one of {RETRY_MODES}, not {retry!r}")
    return retry


def factor_failed(owner, step, enter, call):
    """One pass of updates for the LPs of `step` (active) and of `enter` (entering, the Mehrotra stream).  call(role) -> (rc, fail_col): one
    `tlpk_ipm_batch_factor_each` with role[k] in 0 .. 3; fail_col[k] >= 0 names LP k as failed.  owner: the batched loop (regularisations named by
    `_bumped`, `status`, `timers`, `last_update_rc`, `_call`, `_evict`, `bump_log`, `_last_error`, `_hold_refused`).  Returns what `_factor_enter` returns: (the LPs
    of `step` that hold a factor, the LPs of `enter` whose starting matrix was factorised).

    Round 1 factorises step | enter.  An LP with a verdict is bumped (x 100, the three-bump rule per LP; an entering LP has nothing to bump and
    is out at once); the next call factorises the LPs that failed and still run, holds the LPs that came through, parks the rest.  The loop ends
    with a call that returns TLPK_OK -- after an LP has left, one more call with nothing but holds and parked LPs makes the handle factored.
    Where the library refuses a hold the pass goes on without holds (every LP that would hold is factorised again: the same values, the same
    factor) and the owner is told, once."""
    B = owner.nlp
    step, enter, entering = step.copy(), enter.copy(), enter.copy()
    nbump = np.zeros(B, dtype=np.int64)
    todo = step | enter                                                      # what the next call factorises
    use_hold = True
    while step.any() or enter.any():
        live = step | enter
        role = np.zeros(B, dtype=np.uint8)
        work = todo if use_hold else live
        role[live & ~work] = ROLE_HOLD
        role[work & step] = ROLE_ACTIVE
        role[work & enter] = ROLE_ENTERING
        rc, fail_col = call(role)
        owner.last_update_rc = rc
        if rc == _lib.BADARG and (role == ROLE_HOLD).any() and "hold refused" in owner._last_error():      # (refused before anything ran; any other
            owner._hold_refused()                                            # TLPK_BADARG is an error like everywhere else: `_call` below)
            use_hold = False
            continue
        owner.timers["n_update_calls"] += 1
        owner.timers["n_lp_factor"] += int(work.sum())
        if rc == _lib.OK:
            owner.timers["n_update"][live] += 1
            break
        if rc != _lib.NOT_POSDEF:
            owner._call(rc)
        bad = (np.asarray(fail_col) >= 0) & work
        if not bad.any():
            bad = work.copy()                                                # the pivot cannot be attributed: every LP of the update counts a failure
        for k in np.flatnonzero(bad & enter):                                # (its regularisations are the starting point's constants)
            owner.status[k] = "Trm_NumericalProblem"
            enter[k] = False
            owner._evict(int(k))
        bs = bad & step
        for name in owner._bumped:
            getattr(owner, name)[bs] *= 100
        nbump[bs] += 1
        owner.timers["n_bump"][bs] += 1
        gone = bs & ~(nbump < 3)                                             # step.jl:51 (the reference's off-by-one is kept)
        owner.status[gone] = "Trm_NumericalProblem"
        step &= ~gone
        todo = bs & step
    owner.timers["max_bumps_in_a_step"] = np.maximum(owner.timers["max_bumps_in_a_step"], np.where(entering, 0, nbump))
    if nbump.any():
        owner.bump_log.append(nbump.copy())
    return step, enter


def warn_hold_refused(owner, reason):
    warnings.warn(f"{type(owner).__name__}(retry='failed'): the library refuses to hold a factor ({reason}); falling back to retry='all'",
                  RuntimeWarning, stacklevel=3)


__all__ = ["RETRY_MODES", "check_retry", "factor_failed", "warn_hold_refused"]
