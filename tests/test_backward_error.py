"""Componentwise backward error of the factor and of the solves, for every kind of handle (tests/backward_error.py holds the bounds and
their derivation).  The accuracy checks of the other files are normwise -- max|L - L_oracle| <= 1e-11 max|L|, max|dy - dy_oracle| <= 1e-9 --
and a wrong SMALL entry of the factor or of the solution passes all of them (test_mutation_* below shows it on every input).

CPU: (a) the numpy restatement of the device's algorithm is inside the bound on every input (the guard of the inputs); (b) so is the
factor tests/emulate.py produces from the exported schedule (substitution instead of inverses: pins the host schedule componentwise);
(c) one perturbed small entry passes the old criteria and fails the new.  GPU (-m gpu): update + one solve, the factor read back with
factor_panels(), the device's L, dy, dx through the same checker: omega_hard <= 1 (the theorem) and omega_unit <= 8 max(restatement's, 1).
Every leg prints its statistics; the table of a run on an MI355X is profiles/backward_error.txt."""
import copy
import functools

import numpy as np
import pytest

import tulip_jl_amd as tk
from backward_error import (Allowances, NotFactorisable, System, blocks_of, dense_L_of_emulator, dx_stats, factor_stats, restate,
                            rows_to_check, solve_stats)
from emulate import Emulator, panels_to_dense_L
from helpers import block_angular, ipm_like_data, random_lp_matrix

SEED = 3
RATIO = 8.0            # omega_unit(device) <= RATIO * max(omega_unit(restatement), 1): see "WHY 8" in tests/backward_error.py


def _k1_small():
    return random_lp_matrix(470, 1100, 3, 201), {}


def _k1_wide():
    return random_lp_matrix(1500, 2500, 6, 11), {}


def _k1_block():
    A, rb = block_angular(8, 300, 600, 60, 3, 0.5, 5)
    return A, dict(row_block=rb)


def _k1_single():
    from test_symbolic import singleton_rows_matrix
    return singleton_rows_matrix(), {}


def _k1_slack():
    return random_lp_matrix(700, 500, 4, 5, slack=True), {}


def _k2_random():
    return random_lp_matrix(300, 800, 3, 200), {}


def _k2_block():
    A, rb = block_angular(4, 60, 120, 10, 3, 0.5, 3)
    return A, dict(row_block=rb)


def _dense_cols():
    from test_dense_cols import planted
    A, _ = planted(300, 700, 3, [60 + (7 * t) % 90 for t in range(40)], 70)      # the (300, 700, k = 40) case of tests/test_dense_cols.py
    return A, dict(dense_cols="auto", dense_col_min=40, relax=1)


def _dense(m, n):
    from test_dense_backend import dense_A
    return lambda: (dense_A(m, n, seed=m + n), {})


# name -> (kind of the factored system, backend class, matrix + backend keywords)
INPUTS = {
    "k1_small": ("k1", "sparse", _k1_small),            # small fronts, k_potrf_small, gathers
    "k1_wide": ("k1", "sparse", _k1_wide),              # a front wider than 512: multi-panel potrf / trsm / MFMA update, split-K reduce (row sample)
    "k1_block": ("k1", "sparse", _k1_block),            # root front, extend-add across groups (row sample)
    "k1_single": ("k1", "sparse", _k1_single),          # 1 x 1 fronts
    "k1_slack": ("k1", "sparse", _k1_slack),            # slack columns
    "k2_random": ("k2", "sparse", _k2_random),          # SIGNED instances
    "k2_block": ("k2", "sparse", _k2_block),
    "dense_cols": ("dense_cols", "sparse", _dense_cols),          # augmented nodes, quasi-definite
    "dense_1x5": ("k1", "dense", _dense(1, 5)),         # lda padding
    "dense_100x37": ("k1", "dense", _dense(100, 37)),   # n < m
    "dense_256x512": ("k1", "dense", _dense(256, 512)),
    "dense_333x1001": ("k1", "dense", _dense(333, 1001)),         # split-K SYRK + reduce, K tail n mod 16 = 9, both GEMVs
}
LATE = {"k1_small": "late", "k2_random": "late", "dense_333x1001": "late"}
COMBOS = [(name, reg) for name in INPUTS for reg in ("ones", "mid")] + list(LATE.items())
IDS = [f"{a}-{b}" for a, b in COMBOS]


def data_of(m, n, regime):
    if regime == "late7":                                # late data with every 7th theta^-1 + Rp set to zero: only K2 can take it
        th, rp, rd, xp, xd = ipm_like_data(m, n, SEED, "late")
        th[::7] = 0.0; rp[::7] = 0.0
        return th, rp, rd, xp, xd
    return ipm_like_data(m, n, SEED, regime)


def make_handle(name, device, inputs=None):
    """`inputs`: a table like INPUTS (tests/test_front_shapes.py brings its own)"""
    kind, backend, make = (INPUTS if inputs is None else inputs)[name]
    A, kw = make()
    if backend == "dense":
        return A, tk.setup(A, tk.K1(), tk.DenseBackend(device=device))
    return A, tk.setup(A, tk.K2() if kind == "k2" else tk.K1(), tk.Backend(device=device, **kw))


class Problem:
    """One input and regime: the analysed handle, K^ and the data in long double, the restatement with its statistics."""

    def __init__(self, name, regime, inputs=None):
        self.inputs = INPUTS if inputs is None else inputs
        self.name, self.regime, self.kind = name, regime, self.inputs[name][0]
        self.A, self.kkt = make_handle(name, -1, self.inputs)
        m, n = self.A.shape
        self.data = data_of(m, n, regime)
        self.perm = self.kkt.symbolic("perm")
        dense = self.kkt.symbolic("dense_cols") if self.kind == "dense_cols" else None
        self.system = System(self.kind, self.A, self.perm, self.data, dense)
        self.blocks = blocks_of(self.kkt)
        self.rows = rows_to_check(self.system.N, self.kkt)
        try:
            self.L, self.w = restate(self.system, self.blocks)
            self.stats = self.check("restatement", self.L, self.w)
        except NotFactorisable as e:
            self.L = self.w = None
            self.stats = dict(error=str(e))

    def check(self, who, L, w=None, dxdy=None):
        """The statistics of a factor (and of a solution, permuted or as (dx, dy)); prints the line of the table."""
        allow = Allowances(self.system, L, self.blocks)
        out = dict(factor=factor_stats(allow, self.rows))
        if dxdy is not None:
            w = self.system.permuted(*dxdy)
        if w is not None:
            out["solve"] = solve_stats(allow, w)
            if self.kind != "k2":
                dx, dy = dxdy if dxdy is not None else self.system.unpermuted(w)
                out["dx"] = dx_stats(self.system, dx, dy)
        print(f"BE {self.name:15s} {self.regime:5s} {who:11s} N={self.system.N:5d} rows={len(self.rows):4d} | "
              + " | ".join(f"{k} hard={v['hard']:.3e} unit={v['unit']:.3e}" for k, v in out.items()))
        return out

    def assert_good_input(self):
        assert "error" not in self.stats, f"bad test input {self.name}/{self.regime}: the restatement does not factorise it ({self.stats['error']})"
        for part, v in self.stats.items():
            assert v["hard"] <= 1.0, f"bad test input {self.name}/{self.regime}: the restatement's {part} has omega_hard = {v['hard']:.3e} at {v['at']}"


@functools.lru_cache(maxsize=2)
def problem(name, regime):
    return Problem(name, regime)


@pytest.fixture(scope="module", params=COMBOS, ids=IDS)
def pb(request):
    """Module scope: pytest runs the legs of one input and regime together, so its long-double data is built once."""
    return problem(*request.param)


def emulator_of(pb):
    kind, backend, _ = pb.inputs[pb.name]
    if backend == "dense":
        from test_dense_backend import DenseEmulator
        return DenseEmulator(pb.kkt)
    if kind == "dense_cols":
        from test_set_values import DenseColsEmulator
        return DenseColsEmulator(pb.kkt)
    return Emulator(pb.kkt)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_restatement_is_inside_the_bound(pb):
    """(a) -- the guard of the inputs: the GPU legs assert it first."""
    pb.assert_good_input()


def test_emulated_schedule_is_inside_the_bound(pb):
    """(b): the factor of the exported schedule, executed by tests/emulate.py with substitution."""
    emulator_leg(pb)


def emulator_leg(pb):
    pb.assert_good_input()
    em = emulator_of(pb)
    em.update(*pb.data[:3])
    assert em.fail_col is None
    st = pb.check("emulator", dense_L_of_emulator(em, pb.system.N))
    assert st["factor"]["hard"] <= 1.0, st
    assert st["factor"]["unit"] <= RATIO * max(pb.stats["factor"]["unit"], 1.0), (st, pb.stats)


def small_entry(pb, allow):
    """The below-diagonal entry (i, j) of the checked rows with 0 < |L_ij| < 1e-3 max|L| whose own term |L_ij| |L_jj| is the largest share of
    its allowance: where a relative perturbation of L_ij shows most."""
    L = pb.L
    rows = pb.rows
    share = np.zeros((len(rows), L.shape[1]))
    small = (np.abs(L[rows]) > 0) & (np.abs(L[rows]) < 1e-3 * np.abs(L).max()) & (np.arange(L.shape[1])[None, :] < rows[:, None])
    with np.errstate(divide="ignore", invalid="ignore"):
        share[small] = (np.abs(L[rows]) * np.abs(np.diag(L))[None, :] / allow.hard[rows])[small]
    a, j = np.unravel_index(int(np.argmax(share)), share.shape)
    assert share[a, j] > 0, "no small below-diagonal entry"
    return int(rows[a]), int(j)


def test_mutation_one_small_entry_passes_the_normwise_criteria_and_fails_the_bound(pb):
    """(c): L_ij (1 + 1e-9) for one small entry is invisible to max|L - L_ref| <= 1e-11 max|L|, w_i (1 + 1e-10) to max|w - w_ref| <= 1e-9
    max(1, max|w|) -- the criteria of compare_with_oracle / check_factor_and_solution -- and both break omega_hard <= 1."""
    mutation_leg(pb)


def mutation_leg(pb):
    name, regime = pb.name, pb.regime
    pb.assert_good_input()
    if pb.system.N == 1:                                    # dense_1x5: a 1 x 1 factor has no below-diagonal entry and its solve is one division
        assert pb.L.shape == (1, 1)
        return
    allow = Allowances(pb.system, pb.L, pb.blocks)
    i, j = small_entry(pb, allow)
    Lm = pb.L.copy()
    Lm[i, j] *= 1.0 + 1e-9
    old = np.abs(Lm - pb.L).max() / np.abs(pb.L).max()
    mutated = copy.copy(allow)               # (the allowances move by 1e-9 of themselves: kept)
    mutated.L = Lm
    new = factor_stats(mutated, np.array([i]))
    # the solution: the entry whose column of K^ is the largest share of a row's allowance
    before = solve_stats(allow, pb.w)
    k = int(np.argmax(np.abs(pb.w) * (np.abs(pb.system.K64) / np.maximum(before["allowance"], 1e-300)[:, None]).max(axis=0)))
    wm = pb.w.copy()
    wm[k] *= 1.0 + 1e-10
    old_w = np.abs(wm - pb.w).max() / max(1.0, np.abs(pb.w).max())
    after = solve_stats(allow, wm)
    print(f"BE {name:15s} {regime:5s} mutation    L[{i},{j}] (1 + 1e-9): max|dL|/max|L| = {old:.2e}, omega_hard {pb.stats['factor']['hard']:.3e} -> {new['hard']:.3e} | "
          f"w[{k}] (1 + 1e-10): max|dw| = {old_w:.2e}, omega_hard {before['hard']:.3e} -> {after['hard']:.3e}")
    assert 0 < old <= 1e-11 and new["hard"] > 1.0
    assert 0 < old_w <= 1e-9 and before["hard"] <= 1.0 and after["hard"] > 1.0


def test_the_row_sample_of_the_large_inputs():
    """Above 1100 rows the residual is formed for a sample of rows (each against all its columns): never fewer than 160, the last 64 and the
    block boundaries of the widest front among them."""
    for name in ("k1_wide", "k1_block"):
        A, kkt = make_handle(name, -1)
        N = A.shape[0]
        rows = rows_to_check(N, kkt)
        assert N > 1100 and 160 <= len(rows) < N and set(range(N - 64, N)) <= set(rows.tolist())
        ns, col0 = kkt.symbolic("front_ns"), kkt.symbolic("front_col0")
        s = int(np.argmax(ns))
        assert ns[s] > 64 and {int(col0[s]) + 62, int(col0[s]) + 63, int(col0[s]) + 64, int(col0[s]) + 65} <= set(rows.tolist())
    A, kkt = make_handle("k2_random", -1)
    assert len(rows_to_check(sum(A.shape), kkt)) == 1100


def test_k2_late_data_with_zero_diagonal_entries_is_not_an_input():
    """Late data with every 7th theta^-1 + Rp set to zero: the restatement meets an exactly zero pivot (a variable node that the ordering
    eliminates before any of its constraints), and so would the device (a pivot must carry the sign of its node).  Such an input is used only
    where the restatement factorises it: the K2 row takes the plain late regime instead (exact zeros in theta^-1, Rp = sqrt(eps))."""
    pb = Problem("k2_random", "late7")
    assert "error" in pb.stats and pb.L is None


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def device_leg(pb, who="device", first=None):
    """`first`: (theta, regP, regD) the handle factorises before the data of `pb` -- what the checked factor's storage then held before"""
    name, regime = pb.name, pb.regime
    pb.assert_good_input()
    A, kkt = make_handle(name, 0, pb.inputs)
    for what in ("perm", "front_col0", "front_ns"):
        assert np.array_equal(kkt.symbolic(what), pb.kkt.symbolic(what)), what
    th, rp, rd, xp, xd = pb.data
    if first is not None:
        tk.update(kkt, *first)
    tk.update(kkt, th, rp, rd)
    dx = np.zeros(A.shape[1]); dy = np.zeros(A.shape[0])
    tk.solve(dx, dy, kkt, xp, xd)
    L = panels_to_dense_L(kkt, kkt.factor_panels())
    kkt.close()
    st = pb.check(who, np.tril(L), dxdy=(dx, dy))
    for part, v in st.items():
        assert v["hard"] <= 1.0, f"{name}/{regime} {part}: omega_hard = {v['hard']:.3e} at {v['at']}"
        ref = pb.stats[part]["unit"]
        assert v["unit"] <= RATIO * max(ref, 1.0), f"{name}/{regime} {part}: omega_unit = {v['unit']:.3e}, the restatement's {ref:.3e}"


@pytest.mark.gpu
def test_device_factor_and_solves_are_inside_the_bound(pb):
    device_leg(pb)


@pytest.mark.gpu
def test_device_with_poisoned_storage(monkeypatch):
    """TLPK_POISON=1: the factor storage starts as NaNs, so never-written storage cannot hide in a product (1500 rows, a front wider than 512)."""
    monkeypatch.setenv("TLPK_POISON", "1")
    device_leg(problem("k1_wide", "mid"), who="device+NaN")
