"""The pair of right-hand sides on a matrix-free handle (tests/test_krylov_pair.py), the part that needs no device: an analysis-only handle serves the two
getter names with zeros and answers tlpk_solve2_device with TLPK_NO_DEVICE."""
import numpy as np
import pytest

import tulip_jl_amd as tk
from tulip_jl_amd import _lib
from helpers import random_lp_matrix

HANDLES = [("K1", dict(method="cg")), ("K1", dict(method="cg", precond="jacobi")), ("K2", dict(method="minres")), ("K2", dict(method="minres", precond="jacobi")),
           ("K2", dict(method="tricg"))]


@pytest.mark.parametrize("system,kw", HANDLES)
def test_getters_and_refusal_without_a_device(system, kw):
    A = random_lp_matrix(30, 50, 3, 1)
    kkt = tk.setup(A, tk.K1() if system == "K1" else tk.K2(), tk.KrylovBackend(device=-1, **kw))
    info = kkt.symbolic("krylov_pair")
    assert info.dtype == np.int64 and info.tolist() == [0] * 7
    resid = _lib.symbolic_array_f64(kkt._h, "krylov_pair_resid")
    assert resid.tolist() == [0.0] * 4
    # cap smaller than the length: the length comes back, cap entries are written
    buf = np.full(3, -1, dtype=np.int64)
    assert _lib.lib().tlpk_symbolic_get(kkt._h, b"krylov_pair", _lib.as_p64(buf), 2) == 7 and buf.tolist() == [0, 0, -1]
    # (any non-null addresses: the call must refuse before it touches them)
    assert _lib.lib().tlpk_solve2_device(kkt._h, 8, 8, 8, 8, 8, 8, 8, 8) == _lib.NO_DEVICE
    assert kkt.symbolic("krylov_pair").tolist() == [0] * 7
    kkt.close()
