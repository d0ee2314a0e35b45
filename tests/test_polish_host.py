"""Refinement on demand (tlpk_polish_device, tlpk_polish2_device, tlpk_polish, tlpk_ipm_set_polish) without a device: the exports, the refusals in the
order include/tlpk.h promises, the report keys before a first call, and a guard on the inputs tests/test_polish.py uses on the GPU."""
import os

import numpy as np
import pytest

import tulip_jl_amd as tk
from helpers import ipm_like_data, random_lp_matrix
from oracle_binding import OracleK1, OracleK2
from polish_reference import norms_ld, polish_reference
from tulip_jl_amd import _lib

BADARG, NO_DEVICE = _lib.BADARG, _lib.NO_DEVICE
NEW = ["tlpk_polish_device", "tlpk_polish2_device", "tlpk_polish", "tlpk_ipm_set_polish"]
# (m, n, seed): A = random_lp_matrix(m, n, 3, 77 + seed), data = ipm_like_data(m, n, seed, "late") -- the K2 inputs of the GPU tests
K2_INPUTS = [(300, 800, 3), (400, 1200, 4), (1500, 3200, 3)]


def k2_input(m, n, seed):
    return random_lp_matrix(m, n, 3, 77 + seed), ipm_like_data(m, n, seed, "late")


def k1_input(regime="late"):
    """The input of tests/test_gpu_parity.py::test_iterative_refinement_option."""
    A = random_lp_matrix(1500, 3200, 4, 77)
    return A, ipm_like_data(1500, 3200, 3, regime)


def _handle(kind):
    if kind == "dense":
        return tk.setup(np.asfortranarray(np.random.default_rng(4).standard_normal((6, 10))), tk.K1(), tk.DenseBackend(device=-1))
    A = random_lp_matrix(30, 50, 3, 3)
    if kind == "krylov":
        return tk.setup(A, tk.K1(), tk.KrylovBackend(device=-1))
    return tk.setup(A, tk.K2() if kind == "k2" else tk.K1(), tk.Backend(device=-1))


def _call(name, h, null_at=-1, steps=1):
    """One call with 64-entry vectors behind every pointer (never dereferenced: every call here is refused before); pointer number null_at is NULL."""
    L = _lib.lib()
    if name == "tlpk_ipm_set_polish":
        return L.tlpk_ipm_set_polish(h, steps), []
    keep = [np.ones(64) for _ in range(8 if name == "tlpk_polish2_device" else 4)]
    if name == "tlpk_polish":
        args = [None if k == null_at else _lib.as_pd(v) for k, v in enumerate(keep)]
    else:
        args = [None if k == null_at else v.ctypes.data for k, v in enumerate(keep)]
    return getattr(L, name)(h, *args, steps), keep


def _err(h):
    return _lib.lib().tlpk_last_error(h).decode()


def test_every_new_symbol_is_exported():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    hdr = open(os.path.join(os.path.dirname(_lib.HERE), "include", "tlpk.h")).read()
    for name in NEW:
        assert f"int {name}(tlpk_handle *h" in hdr, name


@pytest.mark.parametrize("name", NEW)
def test_null_handle(name):
    assert _call(name, None)[0] == BADARG


@pytest.mark.parametrize("kind", ["k1", "k2"])
@pytest.mark.parametrize("name", NEW[:3])
def test_refusal_order_on_an_analysis_only_handle(name, kind):
    npointers = 8 if name == "tlpk_polish2_device" else 4
    for null_at in range(npointers):
        kkt = _handle(kind)
        assert _call(name, kkt._h, null_at)[0] == BADARG
        assert _err(kkt._h) == f"{name}: a NULL pointer"
        # (a NULL pointer comes before steps < 0 ...)
        assert _call(name, kkt._h, null_at, steps=-1)[0] == BADARG and _err(kkt._h) == f"{name}: a NULL pointer"
        kkt.close()
    kkt = _handle(kind)
    # ... and steps < 0 before the missing device
    assert _call(name, kkt._h, steps=-1)[0] == BADARG
    assert _err(kkt._h) == f"{name}: steps = -1, must be >= 0"
    for steps in (0, 1, 3):
        assert _call(name, kkt._h, steps=steps)[0] == NO_DEVICE
    kkt.close()


@pytest.mark.parametrize("kind,words", [("krylov", "a matrix-free handle (tlpk_options.krylov)"), ("dense", "a dense-matrix handle (tlpk_create_dense)")])
@pytest.mark.parametrize("name", NEW[:3])
def test_the_kind_of_handle_is_refused_first(name, kind, words):
    kkt = _handle(kind)
    for null_at, steps in ((-1, 1), (0, 1), (-1, -1)):
        assert _call(name, kkt._h, null_at, steps)[0] == BADARG
        assert _err(kkt._h) == f"{name}: single-device handles with a factor only; this is {words}"
    kkt.close()


def test_ipm_set_polish_without_a_device():
    for kind in ("k1", "k2"):
        kkt = _handle(kind)
        for steps in (0, 1, -1):
            assert _call("tlpk_ipm_set_polish", kkt._h, steps=steps)[0] == NO_DEVICE
        kkt.close()
    for kind, words in (("krylov", "a matrix-free handle"), ("dense", "a dense-matrix handle")):
        kkt = _handle(kind)
        assert _call("tlpk_ipm_set_polish", kkt._h)[0] == BADARG
        assert _err(kkt._h) == f"tlpk_ipm_set_polish: single-device handles with a factor and one LP loaded only; this is {words}"
        kkt.close()


@pytest.mark.parametrize("kind", ["k1", "k2", "krylov", "dense"])
def test_the_report_reads_zero_before_a_first_call(kind):
    kkt = _handle(kind)
    cnt, res, nbytes = kkt.symbolic("polish"), kkt.symbolic_f64("polish_resid"), kkt.symbolic("polish_bytes")
    assert cnt.shape == (6,) and not cnt.any()
    assert res.shape == (8,) and not res.any()
    assert nbytes.shape == (1,) and nbytes[0] == 0
    rep = kkt.polish_report()
    assert rep["bytes"] == 0 and all(v == 0 for side in rep["sides"] for v in side.values())
    kkt.close()


def test_python_wrapper_raises_without_a_device():
    kkt = _handle("k2")
    dx = np.zeros(kkt.n); dy = np.zeros(kkt.m)
    with pytest.raises(RuntimeError):          # TLPK_NO_DEVICE
        kkt.polish(dx, dy, np.ones(kkt.m), np.ones(kkt.n))
    with pytest.raises(tk.DimensionMismatch):
        kkt.polish(np.zeros(kkt.n + 1), dy, np.ones(kkt.m), np.ones(kkt.n))
    kkt.close()


def _guard(orc, A, data):
    th, rp, rd, xp, xd = data
    orc.update(th, rp, rd)
    dx, dy = orc.solve(xp, xd)
    before = norms_ld(A, th, rp, rd, xp, xd, dx, dy)
    dx1, dy1, rep = polish_reference(orc.solve, A, th, rp, rd, xp, xd, dx, dy, 1)
    after = norms_ld(A, th, rp, rd, xp, xd, dx1, dy1)
    return before, after, rep


@pytest.mark.parametrize("m,n,seed", K2_INPUTS)
def test_input_guard_k2(m, n, seed):
    """The K2 inputs of the GPU tests leave something to refine, and one guarded step on the CPU oracle (in the ordering of the handle) removes it:
    |r1|inf shrinks by at least 1e3 (natural order gave >= 1.3e4 when the inputs were chosen).  A failure here says the input is bad, not the device."""
    A, data = k2_input(m, n, seed)
    kkt = tk.setup(A, tk.K2(), tk.Backend(device=-1))
    before, after, rep = _guard(OracleK2(A, kkt.perm()), A, data)
    kkt.close()
    print(f"K2 {m} x {n} seed {seed}: |r1| {before[0]:.3e} -> {after[0]:.3e}, |r2| {before[1]:.3e} -> {after[1]:.3e}, {rep}")
    assert rep["accepted"] == 1 and after[0] * 1e3 <= before[0]


def test_input_guard_k1():
    """The same for the K1 input (that of test_iterative_refinement_option)."""
    A, data = k1_input()
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=-1))
    before, after, rep = _guard(OracleK1(A, kkt.perm()), A, data)
    kkt.close()
    print(f"K1: |r1| {before[0]:.3e} -> {after[0]:.3e}, |r2| {before[1]:.3e} -> {after[1]:.3e}, {rep}")
    assert rep["accepted"] == 1 and after[0] * 1e3 <= before[0]
