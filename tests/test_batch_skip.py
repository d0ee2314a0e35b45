"""Batched loops with parked blocks skipped (`tlpk_ipm_batch_skip`; `BatchedDeviceHSD` / `BatchedDeviceMPC(skip_parked=...)`, DESIGN.md section 4b'-s).
With the switch on, the blocks of the LPs a call's `active` mask leaves out are skipped inside the factorisation and the sweeps; every LP must end
with the status, iteration count, vectors and timers of `skip_parked=False`, bit for bit.  The LPs are the mix of test_hsd_batch.py's retry test
(bump, lpex_opt, stair25: they finish in different iterations, and bump takes the per-LP retry path).  What tells the two settings apart is the
factor storage: with the switch on, the panels of an LP's fronts keep the bits of the last update the LP took part in until the run ends; with it
off they are refactorised from the parking values (theta_inv = Rp = Rd = 1) by the next update."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import tulip_jl_amd as tk  # noqa: E402
from tulip_jl_amd import _lib  # noqa: E402
from tulip_jl_amd.hsd_batch import BatchedDeviceHSD  # noqa: E402
from tulip_jl_amd.mpc_batch import BatchedDeviceMPC  # noqa: E402
from tulip_jl_amd.problem import read_free_mps, standard_form  # noqa: E402
from test_block_skip import expected_front_unit, pk_len  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
VECTORS = {"x": 0, "xl": 1, "xu": 2, "zl": 3, "zu": 4, "y": 5}
TIMERS = ("n_update", "n_solve", "n_bump")


def mix():
    return [standard_form(read_free_mps(os.path.join(GOLDEN, name + ".mps"))) for name in ("bump", "lpex_opt", "stair25")]


def unit_index(opt):
    """Per LP: the positions of its fronts' panels in the factor storage (derived on the host, the same for both settings)."""
    kkt = opt.kkt
    loff, lda, ns = (kkt.symbolic(w) for w in ("front_loff", "front_lda", "front_ns"))
    fu = expected_front_unit(kkt, opt.A, opt.row_block, np.repeat(np.arange(opt.nlp), np.diff(opt.col_off)))[:len(loff)]
    return [np.concatenate([np.arange(loff[s], loff[s] + pk_len(int(lda[s]), int(ns[s]))) for s in np.flatnonzero(fu == k)]) for k in range(opt.nlp)]


def traced_run(cls, system, skip):
    """One run; beside the results, per LP that left before the end: its panels after the last update it took part in, after the first update that followed,
    and at the end of the run; and codes 33 - 35 of tlpk_ipm_get at the end."""
    opt = cls(mix(), system=system, device=0, skip_parked=skip)
    assert opt.skip_parked == skip
    idx = unit_index(opt)
    last, nxt = {}, {}
    inner = opt._factor

    def factor(step):
        held = inner(step)
        if step.any() and opt.last_update_rc == _lib.OK:
            F = opt.kkt.factor_panels()
            for k in range(opt.nlp):
                if held[k]:
                    last[k] = F[idx[k]].copy(); nxt.pop(k, None)
                elif k in last and k not in nxt:
                    nxt[k] = F[idx[k]].copy()
        return held

    opt._factor = factor
    opt.optimize()
    F = opt.kkt.factor_panels()
    rec = {"status": [str(s) for s in opt.status], "niter": opt.niter.copy(), "tau": opt.tau.copy(),
           "timers": {name: opt.timers[name].copy() for name in TIMERS},
           "vec": {name: [opt._get(k, code) for k in range(opt.nlp)] for name, code in VECTORS.items()},
           "parking": [opt._get(k, code) for code in (_lib.IPM_THETA, _lib.IPM_REGP, _lib.IPM_REGD) for k in range(opt.nlp)],
           "last": last, "next": nxt, "end": {k: F[idx[k]].copy() for k in range(opt.nlp)},
           "front_skip": len(opt.kkt.symbolic("front_skip"))}
    opt.kkt.close()
    return rec


def assert_same_results(a, b):
    assert a["status"] == b["status"] and np.array_equal(a["niter"], b["niter"])
    assert a["tau"].tobytes() == b["tau"].tobytes()
    for name in TIMERS:
        assert np.array_equal(a["timers"][name], b["timers"][name]), name
    for name in VECTORS:
        for k, (u, v) in enumerate(zip(a["vec"][name], b["vec"][name])):
            assert u.tobytes() == v.tobytes(), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("cls", [BatchedDeviceHSD, BatchedDeviceMPC], ids=["hsd", "mpc"])
@pytest.mark.parametrize("system", ["K1", "K2"])
def test_skipping_parked_blocks_changes_no_result_and_leaves_their_panels(cls, system):
    on, off = traced_run(cls, system, True), traced_run(cls, system, False)
    print(cls.__name__, system, on["status"], on["niter"].tolist(), {k: v.tolist() for k, v in on["timers"].items()})
    assert_same_results(on, off)
    assert len(set(on["niter"].tolist())) > 1                               # the LPs do finish in different iterations
    left = sorted(on["next"])
    assert left and left == sorted(off["next"])                            # LPs that were parked while others continued
    for k in left:
        # the switch on: nothing touched the panels after the LP left; off: the update after it left refactorised them from the parking values
        assert np.array_equal(on["last"][k], on["next"][k], equal_nan=True) and np.array_equal(on["last"][k], on["end"][k], equal_nan=True), k
        assert not np.array_equal(off["last"][k], off["next"][k], equal_nan=True), k
        # until it left, the factor is the same under both settings
        assert np.array_equal(on["last"][k], off["last"][k], equal_nan=True), k
    # codes 33 - 35 of a parked LP read 1 either way (the last update parked every LP that had left), and no mask is in force outside the calls
    for rec in (on, off):
        assert rec["front_skip"] == 0
        for c in range(3):
            for k in left:
                assert (rec["parking"][c * 3 + k] == 1.0).all(), (c, k)
    for u, v in zip(on["parking"], off["parking"]):
        assert u.tobytes() == v.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("system", ["K1", "K2"])
def test_streaming_with_parked_blocks_skipped(system):
    from test_hsd_stream import family
    fam = family(6)
    runs = []
    for skip in (True, False):
        opt = BatchedDeviceHSD(fam[:2], system=system, device=0, skip_parked=skip)
        records = opt.optimize_stream(fam[2:])
        runs.append((records, opt.passes, opt.refills))
        opt.kkt.close()
    (a, pa, ra), (b, pb, rb) = runs
    assert (pa, ra) == (pb, rb) and len(a) == len(b) == 6 and ra > 0
    for q, (u, v) in enumerate(zip(a, b)):
        assert set(u) == set(v)
        for key in u:
            if isinstance(u[key], np.ndarray):
                assert u[key].tobytes() == v[key].tobytes(), (q, key)
            else:
                assert u[key] == v[key], (q, key)


@pytest.mark.gpu
def test_model_front_door_passes_the_switch_through():
    paths = [os.path.join(GOLDEN, name + ".mps") for name in ("lpex_opt", "lpex_freevars", "stair25")]
    on = tk.Model.optimize_batch([tk.Model.load(p) for p in paths], skip_parked=True, device=0)
    off = tk.Model.optimize_batch([tk.Model.load(p) for p in paths], skip_parked=False, device=0)
    for a, b in zip(on, off):
        assert a.status == b.status == "Trm_Optimal"
        assert a.objective_value() == b.objective_value() and (a.inner is None) == (b.inner is None)
        assert a.inner is None or (a.inner.niter == b.inner.niter and a.inner.x.tobytes() == b.inner.x.tobytes())
