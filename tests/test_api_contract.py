"""The C API's refusals, pinned: which code (and which tlpk_last_error text) every update / solve / refine / root / sync entry
point of include/tlpk.h answers to a null handle, to each null pointer, to a handle without a device, to a dense-matrix handle,
to a multi-device parent and to split-phase halves called out of order -- and that a refused call leaves the handle's next
solve unchanged bit for bit.  The tables were recorded from the library as it stood before the solve paths of
csrc/tlpk_api.cpp were folded into one: they are the specification of that refactoring."""
import ctypes

import numpy as np
import pytest

import tulip_jl_amd as tk
from helpers import block_angular, ipm_like_data, random_lp_matrix
from tulip_jl_amd import _lib

OK, BADARG, NO_DEVICE, NOT_FACTORED = _lib.OK, _lib.BADARG, 5, 7

# Arguments after the handle.  p: device pointer (void *), d: host vector (double *), o: double ** out, c: int64 * out, 1 / 0: that int
SIGNATURES = {
    "tlpk_update": "ddd", "tlpk_solve": "dddd",
    "tlpk_update_device": "ppp", "tlpk_update_device_async": "ppp", "tlpk_solve_device": "pppp", "tlpk_solve2_device": "pppppppp",
    "tlpk_sync": "",
    "tlpk_update_local": "ppp", "tlpk_root_panel": "oc", "tlpk_update_finish": "",
    "tlpk_solve_local": "pp", "tlpk_root_rhs": "oc", "tlpk_solve_finish": "ppp",
    "tlpk_solve2_local": "pppp", "tlpk_root_rhs2": "oc", "tlpk_solve2_finish": "pppppp",
    "tlpk_refine_local": "pppp", "tlpk_refine_finish": "pp", "tlpk_root_copy": "10p",
}
MULTI_TEXT = b"multi-device handle: only tlpk_update / tlpk_solve / tlpk_info / tlpk_destroy apply"
SPLIT_TEXT = ": the split-phase calls do not apply to a dense-matrix handle (tlpk_create_dense)"

# Without a device.  Per entry point: the code for a null handle, then per kind of analysis-only handle (sparse K1, K2, tlpk_create_dense) the
# codes for [valid arguments, first pointer null, second pointer null, ...] (the others valid)
NULL_HANDLE = {
    "tlpk_update": 2, "tlpk_solve": 2, "tlpk_update_device": 2, "tlpk_update_device_async": 2, "tlpk_solve_device": 2, "tlpk_solve2_device": 2,
    "tlpk_sync": 2, "tlpk_update_local": 2, "tlpk_root_panel": 2, "tlpk_update_finish": 2, "tlpk_solve_local": 2, "tlpk_root_rhs": 2,
    "tlpk_solve_finish": 2, "tlpk_solve2_local": 2, "tlpk_root_rhs2": 2, "tlpk_solve2_finish": 2, "tlpk_refine_local": 2, "tlpk_refine_finish": 2,
    "tlpk_root_copy": 2,
}
CODES = {}            # filled below: CODES[name][kind]
DENSE_SPLIT = {}      # DENSE_SPLIT[name]: per case of CODES[name]["dense"], whether tlpk_last_error then names the call and says "split-phase"
CODES["tlpk_update"] = {'k1': [5, 2, 2, 2], 'k2': [5, 2, 2, 2], 'dense': [5, 2, 2, 2]}
DENSE_SPLIT["tlpk_update"] = [False, False, False, False]
CODES["tlpk_solve"] = {'k1': [5, 2, 2, 2, 2], 'k2': [5, 2, 2, 2, 2], 'dense': [5, 2, 2, 2, 2]}
DENSE_SPLIT["tlpk_solve"] = [False, False, False, False, False]
CODES["tlpk_update_device"] = {'k1': [5, 2, 2, 2], 'k2': [5, 2, 2, 2], 'dense': [5, 2, 2, 2]}
DENSE_SPLIT["tlpk_update_device"] = [False, False, False, False]
CODES["tlpk_update_device_async"] = {'k1': [5, 2, 2, 2], 'k2': [5, 2, 2, 2], 'dense': [5, 2, 2, 2]}
DENSE_SPLIT["tlpk_update_device_async"] = [False, False, False, False]
CODES["tlpk_solve_device"] = {'k1': [5, 5, 5, 2, 2], 'k2': [5, 5, 5, 2, 2], 'dense': [5, 5, 5, 2, 2]}
DENSE_SPLIT["tlpk_solve_device"] = [False, False, False, False, False]
CODES["tlpk_solve2_device"] = {'k1': [5, 2, 2, 2, 2, 2, 2, 2, 2], 'k2': [5, 2, 2, 2, 2, 2, 2, 2, 2], 'dense': [5, 2, 2, 2, 2, 2, 2, 2, 2]}
DENSE_SPLIT["tlpk_solve2_device"] = [False, False, False, False, False, False, False, False, False]
CODES["tlpk_sync"] = {'k1': [5], 'k2': [5], 'dense': [5]}
DENSE_SPLIT["tlpk_sync"] = [False]
CODES["tlpk_update_local"] = {'k1': [5, 2, 2, 2], 'k2': [5, 2, 2, 2], 'dense': [2, 2, 2, 2]}
DENSE_SPLIT["tlpk_update_local"] = [True, True, True, True]
CODES["tlpk_root_panel"] = {'k1': [5, 2, 2], 'k2': [5, 2, 2], 'dense': [2, 2, 2]}
DENSE_SPLIT["tlpk_root_panel"] = [True, True, True]
CODES["tlpk_update_finish"] = {'k1': [5], 'k2': [5], 'dense': [2]}
DENSE_SPLIT["tlpk_update_finish"] = [True]
CODES["tlpk_solve_local"] = {'k1': [5, 2, 2], 'k2': [5, 2, 2], 'dense': [2, 2, 2]}
DENSE_SPLIT["tlpk_solve_local"] = [True, True, True]
CODES["tlpk_root_rhs"] = {'k1': [5, 2, 2], 'k2': [5, 2, 2], 'dense': [2, 2, 2]}
DENSE_SPLIT["tlpk_root_rhs"] = [True, True, True]
CODES["tlpk_solve_finish"] = {'k1': [5, 2, 2, 2], 'k2': [5, 2, 2, 2], 'dense': [2, 2, 2, 2]}
DENSE_SPLIT["tlpk_solve_finish"] = [True, True, True, True]
CODES["tlpk_solve2_local"] = {'k1': [5, 2, 2, 2, 2], 'k2': [5, 2, 2, 2, 2], 'dense': [2, 2, 2, 2, 2]}
DENSE_SPLIT["tlpk_solve2_local"] = [True, True, True, True, True]
CODES["tlpk_root_rhs2"] = {'k1': [5, 2, 2], 'k2': [5, 2, 2], 'dense': [2, 2, 2]}
DENSE_SPLIT["tlpk_root_rhs2"] = [True, True, True]
CODES["tlpk_solve2_finish"] = {'k1': [5, 2, 2, 2, 2, 2, 2], 'k2': [5, 2, 2, 2, 2, 2, 2], 'dense': [2, 2, 2, 2, 2, 2, 2]}
DENSE_SPLIT["tlpk_solve2_finish"] = [True, True, True, True, True, True, True]
CODES["tlpk_refine_local"] = {'k1': [5, 2, 2, 2, 2], 'k2': [2, 2, 2, 2, 2], 'dense': [2, 2, 2, 2, 2]}
DENSE_SPLIT["tlpk_refine_local"] = [True, True, True, True, True]
CODES["tlpk_refine_finish"] = {'k1': [5, 2, 2], 'k2': [5, 2, 2], 'dense': [2, 2, 2]}
DENSE_SPLIT["tlpk_refine_finish"] = [True, True, True]
CODES["tlpk_root_copy"] = {'k1': [5, 2], 'k2': [5, 2], 'dense': [2, 2]}
DENSE_SPLIT["tlpk_root_copy"] = [True, True]


def _analysis_only(kind):
    """A fresh handle without a device (opt.device = -1), as tests/test_abi.py makes them."""
    if kind == "dense":
        A = np.asfortranarray(np.random.default_rng(4).standard_normal((6, 10)))
        return tk.setup(A, tk.K1(), tk.DenseBackend(device=-1)), A
    A = random_lp_matrix(30, 50, 3, 3)
    return tk.setup(A, tk.K2() if kind == "k2" else tk.K1(), tk.Backend(device=-1)), A


def _arguments(sig, null_at, keep):
    """ctypes arguments for a signature string; the pointer number `null_at` (0-based among the pointers) is null."""
    args, k = [], 0
    for ch in sig:
        if ch in "10":
            args.append(int(ch)); continue
        if k == null_at:
            args.append(None)
        elif ch == "d":
            v = np.ones(64); keep.append(v); args.append(_lib.as_pd(v))
        elif ch == "p":
            v = np.ones(64); keep.append(v); args.append(v.ctypes.data)      # never dereferenced: every call is refused before
        elif ch == "o":
            v = ctypes.c_void_p(); keep.append(v); args.append(ctypes.byref(v))
        else:
            v = np.zeros(1, dtype=np.int64); keep.append(v); args.append(_lib.as_p64(v))
        k += 1
    return args


def _cases(sig):
    return [-1] + list(range(sum(ch not in "10" for ch in sig)))


def _observe(kind, name):
    L, sig = _lib.lib(), SIGNATURES[name]
    codes, texts = [], []
    for null_at in _cases(sig):
        kkt, _ = _analysis_only(kind)                     # a fresh handle per call: tlpk_last_error then speaks of this call alone
        keep = []
        codes.append(getattr(L, name)(kkt._h, *_arguments(sig, null_at, keep)))
        texts.append((name + SPLIT_TEXT).encode() in L.tlpk_last_error(kkt._h))
        kkt.close()
    return codes, texts


def test_the_signature_table_covers_the_header():
    import re
    from test_abi import header_functions
    want = [n for n in header_functions() if re.match(r"tlpk_(update|solve|refine|root|sync)", n)]
    assert sorted(want) == sorted(SIGNATURES) == sorted(NULL_HANDLE) == sorted(CODES)


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_null_handle(name):
    keep = []
    assert getattr(_lib.lib(), name)(None, *_arguments(SIGNATURES[name], -1, keep)) == NULL_HANDLE[name]


@pytest.mark.parametrize("kind", ["k1", "k2", "dense"])
@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_handle_without_device_and_null_pointers(name, kind):
    codes, texts = _observe(kind, name)
    print(name, kind, codes, texts)
    assert codes == CODES[name][kind]
    assert texts == (DENSE_SPLIT[name] if kind == "dense" else [False] * len(codes))


def test_what_the_issue_checked_by_hand():
    """(the spot checks quoted when the table was specified: valid arguments -> TLPK_NO_DEVICE, a null pointer -> TLPK_BADARG)"""
    for kind in ("k1", "k2"):
        for name in ("tlpk_solve_local", "tlpk_update_device", "tlpk_solve2_finish", "tlpk_refine_finish", "tlpk_sync"):
            assert CODES[name][kind][0] == NO_DEVICE and all(c == BADARG for c in CODES[name][kind][1:]), (name, kind)


# ---- on the device ----
def _last(kkt):
    return _lib.lib().tlpk_last_error(kkt._h)


def _refused(kkt, name, args, code, text):
    rc = getattr(_lib.lib(), name)(kkt._h, *args)
    print(name, rc, _last(kkt))
    assert rc == code, (name, rc)
    if text is not None:
        assert _last(kkt) == text, (name, _last(kkt))


@pytest.mark.gpu
def test_split_phase_misuse_is_refused_and_leaves_the_next_solve_unchanged():
    from helpers import DevBuf
    L = _lib.lib()
    A, rb = block_angular(nblocks=4, mk=200, nk=400, m0=40, nnz_in=3, link_prob=0.5, seed=5)
    m, n = A.shape
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=0, row_block=rb))
    th, rp, rd, xp, xd = ipm_like_data(m, n, 2)
    rng = np.random.default_rng(3)
    xp1, xd1 = rng.standard_normal(m), rng.standard_normal(n)
    d_th, d_rp, d_rd, d_xp, d_xd, d_xp1, d_xd1 = (DevBuf(v) for v in (th, rp, rd, xp, xd, xp1, xd1))
    dx, dy, dx1, dy1 = DevBuf(n), DevBuf(m), DevBuf(n), DevBuf(m)
    P = lambda t: t.ptr                                                  # noqa: E731
    # any solve before an update
    hdx, hdy = np.zeros(n), np.zeros(m)
    _refused(kkt, "tlpk_solve", [_lib.as_pd(hdx), _lib.as_pd(hdy), _lib.as_pd(xp), _lib.as_pd(xd)], NOT_FACTORED, None)
    _refused(kkt, "tlpk_solve_device", [P(dx), P(dy), P(d_xp), P(d_xd)], NOT_FACTORED, None)
    _refused(kkt, "tlpk_solve2_device", [P(dx), P(dy), P(d_xp), P(d_xd), P(dx1), P(dy1), P(d_xp1), P(d_xd1)], NOT_FACTORED, None)
    _refused(kkt, "tlpk_solve_local", [P(d_xp), P(d_xd)], NOT_FACTORED, None)
    _refused(kkt, "tlpk_solve_finish", [P(dx), P(dy), P(d_xd)], NOT_FACTORED, None)
    _refused(kkt, "tlpk_solve2_local", [P(d_xp), P(d_xd), P(d_xp1), P(d_xd1)], NOT_FACTORED, None)
    _refused(kkt, "tlpk_refine_local", [P(dx), P(dy), P(d_xp), P(d_xd)], NOT_FACTORED, None)
    kkt.update_device(P(d_th), P(d_rp), P(d_rd))
    kkt.solve_device(P(dx), P(dy), P(d_xp), P(d_xd))
    kkt.solve_device(P(dx1), P(dy1), P(d_xp1), P(d_xd1))
    ref = [t.get() for t in (dx, dy, dx1, dy1)]
    # second halves without their first half
    no_first = {"tlpk_solve_finish": ([P(dx), P(dy), P(d_xd)], BADARG, b"tlpk_solve_finish without a preceding tlpk_solve_local"),
                "tlpk_solve2_finish": ([P(dx), P(dy), P(d_xd), P(dx1), P(dy1), P(d_xd1)], BADARG, b"tlpk_solve2_finish without a preceding tlpk_solve2_local"),
                "tlpk_refine_finish": ([P(dx), P(dy)], BADARG, b"tlpk_refine_finish without a preceding tlpk_refine_local")}
    for name in no_first:
        _refused(kkt, name, *no_first[name])
    # first halves inside an unfinished solve, second halves of another kind than the first half
    pair_local = [P(d_xp), P(d_xd), P(d_xp1), P(d_xd1)]
    refine_local = [P(dx), P(dy), P(d_xp), P(d_xd)]
    assert L.tlpk_solve_local(kkt._h, P(d_xp), P(d_xd)) == OK
    _refused(kkt, "tlpk_solve2_local", pair_local, BADARG, b"tlpk_solve2_local inside an unfinished solve")
    _refused(kkt, "tlpk_refine_local", refine_local, BADARG, b"tlpk_refine_local inside an unfinished solve")
    _refused(kkt, "tlpk_solve2_finish", *no_first["tlpk_solve2_finish"])
    _refused(kkt, "tlpk_refine_finish", *no_first["tlpk_refine_finish"])
    assert L.tlpk_solve_finish(kkt._h, P(dx), P(dy), P(d_xd)) == OK
    assert L.tlpk_solve2_local(kkt._h, *pair_local) == OK
    _refused(kkt, "tlpk_solve2_local", pair_local, BADARG, b"tlpk_solve2_local inside an unfinished solve")
    _refused(kkt, "tlpk_refine_local", refine_local, BADARG, b"tlpk_refine_local inside an unfinished solve")
    _refused(kkt, "tlpk_solve_finish", *no_first["tlpk_solve_finish"])      # tlpk_solve_finish after tlpk_solve2_local
    _refused(kkt, "tlpk_refine_finish", *no_first["tlpk_refine_finish"])
    assert L.tlpk_solve2_finish(kkt._h, P(dx), P(dy), P(d_xd), P(dx1), P(dy1), P(d_xd1)) == OK
    assert L.tlpk_sync(kkt._h) == OK
    assert all(np.array_equal(a, t.get()) for a, t in zip(ref, (dx, dy, dx1, dy1)))
    keep = [DevBuf(v) for v in ref[:2]]                                  # refinement corrects a solution in place: on a copy
    assert L.tlpk_refine_local(kkt._h, P(keep[0]), P(keep[1]), P(d_xp), P(d_xd)) == OK
    _refused(kkt, "tlpk_solve2_local", pair_local, BADARG, b"tlpk_solve2_local inside an unfinished solve")
    _refused(kkt, "tlpk_refine_local", refine_local, BADARG, b"tlpk_refine_local inside an unfinished solve")
    _refused(kkt, "tlpk_solve_finish", *no_first["tlpk_solve_finish"])
    _refused(kkt, "tlpk_solve2_finish", *no_first["tlpk_solve2_finish"])
    assert L.tlpk_refine_finish(kkt._h, P(keep[0]), P(keep[1])) == OK
    assert L.tlpk_sync(kkt._h) == OK
    # and one correct solve of each kind again: the same bits as before the misuse
    out = [DevBuf(sz) for sz in (n, m, n, m)]
    kkt.solve_device(P(out[0]), P(out[1]), P(d_xp), P(d_xd))
    kkt.solve_device(P(out[2]), P(out[3]), P(d_xp1), P(d_xd1))
    assert all(np.array_equal(a, t.get()) for a, t in zip(ref, out))
    out = [DevBuf(sz) for sz in (n, m, n, m)]
    kkt.solve2_device(P(out[0]), P(out[1]), P(d_xp), P(d_xd), P(out[2]), P(out[3]), P(d_xp1), P(d_xd1))
    assert all(np.array_equal(a, t.get()) for a, t in zip(ref, out))
    kkt.close()


@pytest.mark.gpu
def test_every_split_phase_and_device_pointer_call_is_refused_on_a_multi_device_parent():
    from helpers import DevBuf
    A, rb = block_angular(nblocks=4, mk=200, nk=400, m0=40, nnz_in=3, link_prob=0.5, seed=5)
    m, n = A.shape
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=0, row_block=rb, ngpus=2, devices=[0, 0]))
    th, rp, rd, xp, xd = ipm_like_data(m, n, 2)
    tk.update(kkt, th, rp, rd)
    dx0, dy0 = np.zeros(n), np.zeros(m)
    tk.solve(dx0, dy0, kkt, xp, xd)
    bufs = []
    for name, sig in sorted(SIGNATURES.items()):
        if name in ("tlpk_update", "tlpk_solve", "tlpk_sync"):           # what a multi-device handle accepts
            continue
        args = []
        for ch in sig:
            if ch in "10":
                args.append(int(ch))
            elif ch == "p":
                bufs.append(DevBuf(max(m, n))); args.append(bufs[-1].ptr)
            elif ch == "o":
                bufs.append(ctypes.c_void_p()); args.append(ctypes.byref(bufs[-1]))
            else:
                bufs.append(np.zeros(1, dtype=np.int64)); args.append(_lib.as_p64(bufs[-1]))
        _refused(kkt, name, args, BADARG, MULTI_TEXT)
    assert _lib.lib().tlpk_sync(kkt._h) == OK
    dx1, dy1 = np.zeros(n), np.zeros(m)
    tk.solve(dx1, dy1, kkt, xp, xd)
    assert np.array_equal(dx0, dx1) and np.array_equal(dy0, dy1)
    kkt.close()


@pytest.mark.gpu
def test_a_host_pointer_solve_between_two_resident_pairs_changes_no_bit():
    """Two shards of a multi-device K1 handle on one GPU, driven through the device-resident HSD loop's paired solve
    (tlpk_ipm_hsolve_newton).  tlpk_solve on the same handle publishes every shard's result into the lead's vectors; what it
    needs for that must not reach the next resident pair: same scalars, and after the step the same iterate, bit for bit."""
    from test_hsd_device import _block_angular_lp_data
    from tulip_jl_amd.hsd_device import DeviceHSD
    A, rb, b, c, l, u, _ = _block_angular_lp_data()
    m, n = A.shape
    opt = DeviceHSD(A, b, c, l, u, system="K1", device=0, row_block=rb, ngpus=2, devices=[0, 0])
    L, h = opt.L, opt.kkt._h
    rng = np.random.default_rng(11)
    xp, xd = rng.standard_normal(m), rng.standard_normal(n)

    def pair():
        sc = np.array([opt.tau, opt.kappa, opt.regG, opt.rg, -opt.tau * opt.kappa, 0.0, 0.0, 0.0])
        out = np.zeros(16)
        opt._call(L.tlpk_ipm_hsolve_newton(h, _lib.as_pd(sc), _lib.as_pd(out)))
        return out[:4].copy()

    def step(with_host_solve):
        opt._call(L.tlpk_ipm_reset(h))
        opt.tau = opt.kappa = 1.0
        opt.compute_residuals()
        opt._call(L.tlpk_ipm_factor(h, 1e-3, 1e-3))
        scalars = [pair()]
        if with_host_solve:
            dx, dy = np.zeros(n), np.zeros(m)
            tk.solve(dx, dy, opt.kkt, xp, xd)
            assert np.isfinite(dx).all() and np.isfinite(dy).all()
            scalars.append(pair())
        out = np.zeros(16)
        opt._call(L.tlpk_ipm_advance(h, 0.5, _lib.as_pd(out)))
        return scalars, [opt._get(k, n if k < 5 else m) for k in range(6)], out[0]

    s0, v0, g0 = step(False)               # no host-pointer solve has run on this handle yet
    s1, v1, g1 = step(True)
    print("pair scalars:", s0, s1)
    assert np.array_equal(s0[0], s1[0]) and np.array_equal(s1[0], s1[1])
    assert g0 == g1 and all(np.array_equal(a, b_) for a, b_ in zip(v0, v1))
    opt.kkt.close()
