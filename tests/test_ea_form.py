"""Formed fronts (TLPK_EA_FORM): a gathered front whose panel columns all belong to k_ea_gather is not zero-filled -- the kernel
starts every segment of a panel column from zeros and the entries k_assemble stored in it, and writes every stored double of the column.

CPU (analyse-only handles): which fronts are formed, from the task list; for every formed front, panel column and segment the exported rows of the assembled
entries against the ascending rows that `s_target`, `front_loff` and the packed layout give (numpy, independent of the library's construction); the hashed
schedule arrays do not depend on the knob and the new arrays are empty with TLPK_EA_FORM=0.  The edge shapes the kernel has a branch for are asserted to
occur in the inputs.

GPU: a handle created with TLPK_EA_FORM=1 against one with TLPK_EA_FORM=0, every parent front gathered, after three updates with different
(theta, regP, regD) on each handle -- from the second update on a formed panel holds the previous factor, not zeros: every stored double of every panel
(padding rows included) and one solve bit for bit, with and without TLPK_POISON=1 -- with the poison the whole factor storage, without it the panels
only: the few doubles between two panels are written by no kernel and hold what the allocation held; one block skipped; row bands (TLPK_EA_BANDS) take
the zero-filled path."""
import contextlib
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import tulip_jl_amd as tk  # noqa: E402
from helpers import ipm_like_data, load_golden, random_lp_matrix  # noqa: E402
from test_ea_gather import HASHED, ba8, same, stair25  # noqa: E402

KNOBS = ("TLPK_EA_GATHER", "TLPK_EA_GATHER_MIN_CHILD", "TLPK_EA_GATHER_CAP", "TLPK_POISON", "TLPK_EA_FORM")
NEW = ("ea_form", "ea_gather_asm_ptr", "ea_gather_asm_row")


@contextlib.contextmanager
def knobs(form, cap=None, poison=False):
    """the environment of ONE handle's creation: every parent front with a child is gathered; form 0 = all of them zero-filled, 1 = formed where possible,
    None = TLPK_EA_FORM unset (the default: as 1)"""
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ["TLPK_EA_GATHER"] = "1"
    os.environ["TLPK_EA_GATHER_MIN_CHILD"] = "1"
    if form is not None:
        os.environ["TLPK_EA_FORM"] = str(int(form))
    if cap is not None:
        os.environ["TLPK_EA_GATHER_CAP"] = str(cap)
    if poison:
        os.environ["TLPK_POISON"] = "1"
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def pk_off(lda, col):
    """offset of the virtual row 0 of panel column `col` (packed panels: 64-column slices, slice b stores the rows from 64 b down)"""
    b = col >> 6
    return col * lda - 64 * b * (col - 32 * b - 31)


def cpu_cases():
    A, rb = ba8()
    out = {"ba8": (A, tk.K1(), dict(row_block=rb), None), "ba8-cap256": (A, tk.K1(), dict(row_block=rb), 256), "ba8-cap64": (A, tk.K1(), dict(row_block=rb), 64),
           "ba8-k2": (A, tk.K2(), dict(row_block=rb), None), "ba8-rank1of2": (A, tk.K1(), dict(row_block=rb, rank=1, nranks=2), None),
           "stair25": (stair25(), tk.K1(), {}, None), "stair25-cap3": (stair25(), tk.K1(), {}, 3)}
    for g in load_golden():
        out[f"golden-{g['name']}"] = (g["A_csc"], tk.K1(), {}, None)
    return out


def expected_formed(g):
    """gathered, not a k_front_assemble front, none of its extend-add tasks a row band, and the tasks of its panel part cover the pivot columns"""
    base, fa, ns = g("ea_gather_base"), g("front_fa"), g("front_ns")
    tasks = g("ea_tasks").reshape(-1, 6)
    banded = np.zeros(len(base), dtype=bool)
    covered = np.zeros(len(base), dtype=np.int64)
    for front, j0, j1, _bidx, _br0, br1 in tasks:
        if br1 != 0:
            banded[front] = True
        elif j1 <= ns[front]:
            covered[front] += j1 - j0
    return (base >= 0) & (fa == 0) & ~banded & (covered == ns)


def expected_rows(g, formed, cap):
    """(asm_ptr, asm_row) from the assembly targets: entry e of pivot column tc of front s sits in row s_target[e] - front_loff[s] - pk_off(lda, tc) of the
    front, that is in segment (row - tc) // cap of the column; rows of a segment ascending, counted from the segment's first row"""
    base, col, ptr = g("ea_gather_base"), g("ea_gather_col"), g("ea_gather_ptr")
    loff, lda, f, ns, col0 = (g(w) for w in ("front_loff", "front_lda", "front_f", "front_ns", "front_col0"))
    sp_, tgt = g("s_colptr"), g("s_target")
    nseg = len(ptr) - 1
    segs, rows = [], []
    for s in np.flatnonzero(formed):
        tcs = np.arange(int(ns[s]))
        cnt = np.diff(sp_[col0[s]:col0[s] + ns[s] + 1])
        e = np.arange(sp_[col0[s]], sp_[col0[s] + ns[s]])
        tc = np.repeat(tcs, cnt)
        row = tgt[e] - loff[s] - pk_off(int(lda[s]), tc)
        assert (row >= tc).all() and (row < f[s]).all()
        pc = (row - tc) // cap
        segs.append(col[base[s] + tc] + pc)
        rows.append(row - tc - pc * cap)
    segs, rows = np.concatenate(segs), np.concatenate(rows)
    order = np.lexsort((rows, segs))
    want_ptr = np.zeros(nseg + 1, dtype=np.int64)
    np.cumsum(np.bincount(segs, minlength=nseg), out=want_ptr[1:])
    return want_ptr, rows[order]


@functools.lru_cache(maxsize=None)
def analysed(name):
    """One case analysed with TLPK_EA_FORM 1 and 0: the checks of the index, and which edge shapes the case contains."""
    A, system, kw, cap = cpu_cases()[name]
    with knobs(1, cap):
        kkt = tk.setup(A, system, tk.Backend(device=-1, **kw))
    with knobs(0, cap):
        plain = tk.setup(A, system, tk.Backend(device=-1, **kw))
    with knobs(None, cap):
        dflt = tk.setup(A, system, tk.Backend(device=-1, **kw))
    g = kkt.symbolic
    for w in HASHED + ["ea_gather_base", "ea_gather_col", "ea_gather_ptr", "ea_gather_ent", "ea_gather_launches"]:      # the knob moves none of them
        assert np.array_equal(g(w), plain.symbolic(w)), w
    for w in NEW:
        assert plain.symbolic(w).size == 0, w                     # nothing is built with 0
        assert np.array_equal(g(w), dflt.symbolic(w)), w          # unset = 1
    formed = expected_formed(g)
    flags = dict(formed=int(formed.sum()), empty=False, asm_only=False, mid_slice=False, padded=False)
    if not formed.any():
        for w in NEW:
            assert g(w).size == 0, w
        return flags
    assert np.array_equal(g("ea_form") != 0, formed)
    slice_cap = int(g("ea_gather_cap")[0])
    want_ptr, want_row = expected_rows(g, formed, slice_cap)
    got_ptr, got_row = g("ea_gather_asm_ptr"), g("ea_gather_asm_row")
    assert np.array_equal(got_ptr, want_ptr)
    assert np.array_equal(got_row, want_row)
    assert got_row.size > 0 and got_row.max() < slice_cap
    # every pivot column of a formed front has its diagonal entry: the first row of its first segment
    base, col, ptr = g("ea_gather_base"), g("ea_gather_col"), g("ea_gather_ptr")
    f, ns, lda = g("front_f"), g("front_ns"), g("front_lda")
    panel = np.zeros(len(ptr) - 1, dtype=bool)                    # segments of the formed fronts' panel columns
    for s in np.flatnonzero(formed):
        first = col[base[s]:base[s] + ns[s]]
        assert (np.diff(got_ptr)[first] > 0).all() and (got_row[got_ptr[first]] == 0).all()
        panel[col[base[s]]:col[base[s] + ns[s]]] = True
    assert (np.diff(got_ptr)[~panel] == 0).all()                  # no list for the U part nor for fronts that are not formed
    ncontrib, nasm = np.diff(ptr), np.diff(got_ptr)
    flags["empty"] = bool((panel & (ncontrib == 0) & (nasm == 0)).any())
    flags["asm_only"] = bool((panel & (ncontrib == 0) & (nasm > 0)).any())
    flags["mid_slice"] = bool((ns[formed] > 65).any())            # a column tc > 64 with tc % 64 != 0: rows of its slice above the diagonal
    flags["padded"] = bool((lda[formed] > f[formed]).any())
    return flags


@pytest.mark.parametrize("name", list(cpu_cases()))
def test_assembled_rows_per_segment_follow_from_the_targets(name):
    flags = analysed(name)
    if name.startswith("ba8") or name.startswith("stair25"):
        assert flags["formed"] > 0


def test_the_inputs_contain_the_edge_shapes():
    """a segment with neither contributor nor assembled entry, one with assembled entries only, a column in the middle of a 64-column slice, a padded front"""
    seen = {k: [n for n in cpu_cases() if analysed(n)[k]] for k in ("empty", "asm_only", "mid_slice", "padded")}
    for k, names in seen.items():
        assert names, k


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def step_data(m, n, seed):
    """theta, regP, regD, xi_p, xi_d of update `seed`: all three of the update's vectors differ from update to update"""
    th, rp, rd, xp, xd = ipm_like_data(m, n, seed)
    return th, rp * (1 + seed), rd * (1 + 2 * seed), xp, xd


def stored_mask(kkt):
    """The doubles of the factor storage that belong to a panel: per front and 64-column slice the rows from the slice's first row down to lda, padding rows
    included.  The few doubles between panels (every big panel starts on a cache line) are written by no kernel and hold whatever the allocation held."""
    g = kkt.symbolic
    loff, lda, ns = g("front_loff"), g("front_lda"), g("front_ns")
    mask = np.zeros(kkt.stats()["nnzL_stored"], dtype=bool)
    for s in range(len(loff)):
        for c0 in range(0, int(ns[s]), 64):
            first = int(loff[s]) + pk_off(int(lda[s]), c0) + c0
            mask[first:first + min(64, int(ns[s]) - c0) * (int(lda[s]) - c0)] = True
    return mask


def one_handle(A, system, kw):
    kkt = tk.setup(A, system, tk.Backend(device=0, **kw))
    try:
        m, n = kkt.m, kkt.n
        for seed in (0, 1, 2):
            th, rp, rd, xp, xd = step_data(m, n, seed)
            tk.update(kkt, th, rp, rd)
        dx = np.zeros(n); dy = np.zeros(m)
        tk.solve(dx, dy, kkt, xp, xd)
        return [kkt.factor_panels().copy(), dx, dy], int((kkt.symbolic("ea_form") != 0).sum()), stored_mask(kkt)
    finally:
        kkt.close()


def sharded(A, kw):
    from test_set_values import sharded_step
    ks = [tk.setup(A, tk.K1(), tk.Backend(device=0, rank=r, nranks=2, **kw)) for r in range(2)]
    try:
        m, n = ks[0].m, ks[0].n
        for seed in (0, 1, 2):
            out = sharded_step(ks, step_data(m, n, seed))
        raw = [k.factor_panels().copy() for k in ks]
        return [np.concatenate(raw), out[1], out[2]] + out, sum(int((k.symbolic("ea_form") != 0).sum()) for k in ks), np.concatenate([stored_mask(k) for k in ks])
    finally:
        for k in ks:
            k.close()


def gpu_cases():
    A, rb = ba8()
    return {"ba8-k1": (A, tk.K1(), dict(row_block=rb), None), "ba8-cap256": (A, tk.K1(), dict(row_block=rb), 256), "ba8-cap64": (A, tk.K1(), dict(row_block=rb), 64),
            "ba8-k2": (A, tk.K2(), dict(row_block=rb), None), "ba8-ranks": (A, None, dict(row_block=rb), None),
            "stair25": (stair25(), tk.K1(), {}, None), "stair25-cap3": (stair25(), tk.K1(), {}, 3), "golden": (None, tk.K1(), {}, None)}


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poison"])
@pytest.mark.parametrize("name", list(gpu_cases()))
def test_gpu_formed_factor_and_solve_equal_the_zero_filled_ones_bitwise(name, poison):
    A, system, kw, cap = gpu_cases()[name]
    mats = [g["A_csc"] for g in load_golden()] if name == "golden" else [A]
    formed = 0
    for M in mats:
        res, mask = {}, {}
        for form in (0, 1):
            with knobs(form, cap, poison):
                res[form], nform, mask[form] = sharded(M, kw) if system is None else one_handle(M, system, kw)
            if form == 0:
                assert nform == 0
            else:
                formed += nform
        assert all(np.isfinite(x).all() for x in res[1][1:3])         # (dx, dy)
        assert np.array_equal(mask[0], mask[1])
        if poison:
            assert same(res[1], res[0]), name                         # the whole factor storage (what no kernel writes holds the poison) and the solve
        # every stored double of every panel, padding rows included, and the solve (without the poison the doubles between panels are the allocation's)
        assert same([res[1][0][mask[1]]] + res[1][1:], [res[0][0][mask[0]]] + res[0][1:]), name
    assert formed > 0 or name == "golden"                             # (the golden LPs are too small for a parent front to be certain)


@functools.lru_cache(maxsize=None)
def diag3():
    """three independent blocks (row_block = block index): what tlpk_block_skip takes"""
    mats = [random_lp_matrix(420, 700, 6, 11 + k) for k in range(3)]
    A = sp.block_diag(mats, format="csc")
    A.sort_indices()
    return A, np.repeat(np.arange(3), 420).astype(np.int64)


@pytest.mark.gpu
def test_gpu_a_skipped_block_is_neither_zeroed_nor_formed():
    from test_block_skip import pk_len
    A, rb = diag3()
    m, n = A.shape
    out = {}
    for form in (0, 1):
        with knobs(form):
            kkt = tk.setup(A, tk.K1(), tk.Backend(device=0, row_block=rb))
        try:
            th, rp, rd, xp, xd = step_data(m, n, 0)
            tk.update(kkt, th, rp, rd)
            F0 = kkt.factor_panels().copy()
            tk.block_skip(kkt, [0, 1, 0])
            th, rp, rd, xp, xd = step_data(m, n, 1)
            tk.update(kkt, th, rp, rd)
            F1 = kkt.factor_panels().copy()
            loff, lda, ns = (kkt.symbolic(w) for w in ("front_loff", "front_lda", "front_ns"))
            fu = kkt.symbolic("front_unit")[:len(loff)]
            tk.block_skip(kkt, None)
            nform = kkt.symbolic("ea_form")
            assert (form == 0 and nform.size == 0) or (form == 1 and (nform[fu == 1] != 0).any())      # the skipped block has formed fronts
            idx = [np.concatenate([np.arange(loff[s], loff[s] + pk_len(int(lda[s]), int(ns[s]))) for s in np.flatnonzero(fu == u)]) for u in range(3)]
            assert np.array_equal(F1[idx[1]], F0[idx[1]]), "the skipped block's panels were touched"
            assert not np.array_equal(F1[idx[0]], F0[idx[0]]) and not np.array_equal(F1[idx[2]], F0[idx[2]])
            mask = stored_mask(kkt)
            out[form] = [F0[mask], F1[mask]]                  # (the doubles between panels are the allocation's)
        finally:
            kkt.close()
    assert same(out[1], out[0])


BANDS_CHILD = r"""
import os, sys
import numpy as np
sys.path[:0] = [{here!r}, {root!r}]
import tulip_jl_amd as tk
from test_ea_form import expected_formed, knobs, one_handle
from test_ea_gather import gs2600, same
A = gs2600()
with knobs(1):
    g = tk.setup(A, tk.K1(), tk.Backend(device=-1)).symbolic
tasks = g("ea_tasks").reshape(-1, 6)
banded = np.unique(tasks[tasks[:, 5] != 0, 0])
assert banded.size > 0 and (g("front_f")[banded] >= 2048).all()
form = g("ea_form")
assert form.size == 0 or not form[banded].any()                      # a front with a row-band task keeps the zero-filled path ...
assert np.array_equal(form != 0, expected_formed(g)) if form.size else not expected_formed(g).any()
zt = g("zero_tasks").reshape(-1, 2)
assert np.isin(banded, zt[:, 0]).all()                               # ... and its zero-fill tasks
res, mask = {{}}, {{}}
for f in (0, 1):
    with knobs(f):
        res[f], _, mask[f] = one_handle(A, tk.K1(), {{}})
assert all(np.isfinite(x).all() for x in res[1][1:3]) and np.array_equal(mask[0], mask[1])
assert same([res[1][0][mask[1]]] + res[1][1:], [res[0][0][mask[0]]] + res[0][1:])
print("bands ok")
"""


@pytest.mark.gpu
def test_gpu_row_bands_take_the_zero_filled_path():
    """TLPK_EA_BANDS is read by the first analysis of a process: a child process of its own, on the general sparse LP whose top front has 2048 rows or more"""
    env = dict(os.environ)
    for k in KNOBS:
        env.pop(k, None)
    env["TLPK_EA_BANDS"] = "2"
    r = subprocess.run([sys.executable, "-c", BANDS_CHILD.format(here=HERE, root=ROOT)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bands ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
