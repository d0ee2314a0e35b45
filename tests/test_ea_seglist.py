"""Flat segment list of the formed fronts' panel columns (k_ea_seglist, TLPK_EA_SEGLIST): one record per (formed front, panel column,
segment) in the order extend-add launch -> front -> column -> segment, with everything the kernel needs of the segment; a wave walks a run of consecutive
records of its launch's range.

CPU (analyse-only handles): the records are exactly the segments of the panel columns of the formed fronts, each once, in that order; every field against
values recomputed in numpy from `ea_gather_col`, `ea_gather_ptr`, `ea_gather_asm_ptr`, `front_loff`, `front_lda`, `front_f` and the packed-panel offset
(nothing of the library's construction is reused); the launch ranges partition the list; with TLPK_EA_SEGLIST=0 the new arrays are empty and no other
exported array differs.  The shapes the kernel has a path for are asserted to occur in the inputs.

GPU: a handle created with TLPK_EA_SEGLIST=1 against one with 0 (both with every parent front gathered and formed where possible), three updates with
different (theta, regP, regD) on each and one solve, bit for bit: with TLPK_POISON=1 the whole factor storage, without it every stored double of every
panel, padding rows included; one variant with a block skipped."""
import contextlib
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import tulip_jl_amd as tk  # noqa: E402
from test_ea_form import NEW as FORM_ARRAYS, diag3, knobs, pk_off, step_data, stored_mask  # noqa: E402
from test_ea_gather import HASHED, ba8, same, stair25  # noqa: E402

LK_EXTEND_ADD = 0
NEW = ("ea_seg_rec", "ea_seg_launch")
FIELDS = ("front", "dst", "n", "r0", "e0", "ne", "a0", "na", "za", "zb")
EG_EB, EG_CH = 8, 2            # kernels.hip: contributors per batch; a contributor of more than EG_CH x 64 rows takes the thick path


@contextlib.contextmanager
def seg_knobs(seglist, cap=None, poison=False):
    """the environment of ONE handle's creation: test_ea_form's (every parent front gathered, formed where possible) and TLPK_EA_SEGLIST = 0 | 1 | unset (None)"""
    saved = os.environ.pop("TLPK_EA_SEGLIST", None)
    if seglist is not None:
        os.environ["TLPK_EA_SEGLIST"] = str(int(seglist))
    try:
        with knobs(1, cap, poison):
            yield
    finally:
        os.environ.pop("TLPK_EA_SEGLIST", None)
        if saved is not None:
            os.environ["TLPK_EA_SEGLIST"] = saved


def cases():
    A, rb = ba8()
    return {"ba8": (A, dict(row_block=rb), None), "ba8-cap256": (A, dict(row_block=rb), 256), "ba8-cap64": (A, dict(row_block=rb), 64),
            "stair25-cap3": (stair25(), {}, 3)}


def expected_records(g):
    """(records, launches) from the exported index: per extend-add launch, in task order, the panel-part tasks of the formed fronts; per task its columns; per
    column tc its segments g = col[tc] .. col[tc + 1]: rows [r0, r0 + n) of the front, r0 = tc + (g - col[tc]) cap, stored from
    loff + pk_off(lda, tc) + r0 on; the first one zeroes the tc % 64 rows its slice stores above the diagonal, the last one the lda - f padding rows"""
    base, col, ptr, aptr = g("ea_gather_base"), g("ea_gather_col"), g("ea_gather_ptr"), g("ea_gather_asm_ptr")
    loff, lda, f, ns = g("front_loff"), g("front_lda"), g("front_f"), g("front_ns")
    cap = int(g("ea_gather_cap")[0])
    formed = g("ea_form") != 0
    tasks = g("ea_tasks").reshape(-1, 6)
    recs, launches = [], []
    nrec = 0
    for kind, first, count in g("factor_launches").reshape(-1, 3):
        if kind != LK_EXTEND_ADD:
            continue
        s0 = nrec
        for front, j0, j1, _bidx, _br0, br1 in tasks[first:first + count]:
            if not formed[front] or br1 != 0 or j0 >= ns[front]:
                continue
            assert j1 <= ns[front]
            tc = np.arange(j0, j1)
            g0, g1 = col[base[front] + tc], col[base[front] + tc + 1]
            cnt = g1 - g0
            seg = np.concatenate([np.arange(a, b) for a, b in zip(g0, g1)])
            tcs, first_seg, last_seg = np.repeat(tc, cnt), np.repeat(g0, cnt), np.repeat(g1 - 1, cnt)
            r0 = tcs + (seg - first_seg) * cap
            n = np.minimum(cap, f[front] - r0)
            assert (n > 0).all()
            dst = loff[front] + pk_off(int(lda[front]), tcs) + r0
            za = np.where(seg == first_seg, tcs & 63, 0)
            zb = np.where(seg == last_seg, lda[front] - f[front], 0)
            recs.append(np.stack([np.full(len(seg), front), dst, n, r0, ptr[seg], ptr[seg + 1] - ptr[seg], aptr[seg], aptr[seg + 1] - aptr[seg], za, zb, seg], axis=1))
            nrec += len(seg)
        if nrec > s0:
            launches.append((first, s0, nrec))
    recs = np.concatenate(recs) if recs else np.zeros((0, 11), dtype=np.int64)
    return recs, np.array(launches, dtype=np.int64).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def analysed(name):
    """One case analysed with TLPK_EA_SEGLIST 1, 0 and unset: the checks of the list, and the shapes the case contains."""
    A, kw, cap = cases()[name]
    with seg_knobs(1, cap):
        kkt = tk.setup(A, tk.K1(), tk.Backend(device=-1, **kw))
    with seg_knobs(0, cap):
        off = tk.setup(A, tk.K1(), tk.Backend(device=-1, **kw))
    with seg_knobs(None, cap):
        dflt = tk.setup(A, tk.K1(), tk.Backend(device=-1, **kw))
    g = kkt.symbolic
    for w in HASHED + ["ea_gather_base", "ea_gather_col", "ea_gather_ptr", "ea_gather_ent", "ea_gather_cap", "ea_gather_launches"] + list(FORM_ARRAYS):
        assert np.array_equal(g(w), off.symbolic(w)), w               # the knob moves no other exported array
    for w in NEW:
        assert off.symbolic(w).size == 0, w                           # nothing is built with 0
        assert np.array_equal(g(w), dflt.symbolic(w)), w              # unset = 1
    want, want_launch = expected_records(g)
    got, got_launch = g("ea_seg_rec").reshape(-1, len(FIELDS)), g("ea_seg_launch").reshape(-1, 3)
    assert len(got) > 0
    for k, w in enumerate(FIELDS):
        assert np.array_equal(got[:, k], want[:, k]), w
    # exactly the segments of the panel columns of the formed fronts, each once
    base, col, ns = g("ea_gather_base"), g("ea_gather_col"), g("front_ns")
    formed = np.flatnonzero(g("ea_form") != 0)
    panel = np.concatenate([np.arange(col[base[s]], col[base[s] + ns[s]]) for s in formed])
    assert len(np.unique(want[:, 10])) == len(want) and np.array_equal(np.sort(want[:, 10]), np.sort(panel))
    # the launch ranges partition the list, in launch order
    assert np.array_equal(got_launch, want_launch)
    assert got_launch[0, 1] == 0 and got_launch[-1, 2] == len(got) and np.array_equal(got_launch[1:, 1], got_launch[:-1, 2]) and (got_launch[:, 2] > got_launch[:, 1]).all()
    assert (np.diff(got_launch[:, 0]) > 0).all()
    rec = {w: got[:, k] for k, w in enumerate(FIELDS)}
    # what the records write -- [dst - za, dst + n + zb) -- is every stored double of the formed fronts' panels once, and nothing else
    loff, lda = g("front_loff"), g("front_lda")
    cover = np.zeros(kkt.stats()["nnzL_stored"] + 1, dtype=np.int64)
    np.add.at(cover, rec["dst"] - rec["za"], 1)
    np.add.at(cover, rec["dst"] + rec["n"] + rec["zb"], -1)
    cover = np.cumsum(cover)[:-1]
    want_cover = np.zeros(len(cover), dtype=np.int64)
    for s in formed:
        for c0 in range(0, int(ns[s]), 64):
            first = int(loff[s]) + pk_off(int(lda[s]), c0) + c0
            want_cover[first:first + min(64, int(ns[s]) - c0) * (int(lda[s]) - c0)] = 1
    assert np.array_equal(cover, want_cover)
    ent_all, arow_all = g("ea_gather_ent").reshape(-1, 4), g("ea_gather_asm_row")
    assert (rec["e0"] >= 0).all() and (rec["e0"] + rec["ne"] <= len(ent_all)).all() and (rec["a0"] >= 0).all() and (rec["a0"] + rec["na"] <= len(arow_all)).all()
    assert (rec["na"] <= rec["n"]).all()
    slice_rows = {int(first): int(rows) for first, _ng, _np, rows in g("ea_gather_launches").reshape(-1, 4)}
    assert all(rec["n"][s0:s1].max() <= slice_rows[int(first)] for first, s0, s1 in got_launch)                             # a segment fits its launch's LDS slice
    # shapes
    chunk = int(g("ea_seg_chunk")[0])
    ent_rows = g("ea_gather_ent").reshape(-1, 4)[:, 2]
    assert (ent_rows >= 1).all()                                      # the kernel's cursor over a batch relies on it: every contributor has a row
    rows_max = np.array([ent_rows[a:a + c].max() if c else 0 for a, c in zip(rec["e0"], rec["ne"])])
    # thick batches (a contributor of more than EG_CH x 64 rows among the EG_EB): those with more than one contributor -- the cursor moves on to the next
    # contributor --, and those with a contributor of more than one trip of 4 x 64 rows -- the cursor moves inside it
    thick_many = thick_long = 0
    for a, c in zip(rec["e0"][rows_max > 64 * EG_CH], rec["ne"][rows_max > 64 * EG_CH]):
        for b0 in range(int(a), int(a + c), EG_EB):
            nb = ent_rows[b0:min(b0 + EG_EB, int(a + c))]
            if nb.max() > 64 * EG_CH:
                thick_many += int(len(nb) > 1)
                thick_long += int(nb.max() > 256)
    per_col = np.concatenate([np.diff(col[base[s]:base[s] + ns[s] + 1]) for s in formed])                    # segments per panel column
    assert per_col.sum() == len(got)
    nwaves = -(-(got_launch[:, 2] - got_launch[:, 1]) // chunk)
    two_fronts = 0
    for _first, s0, s1 in got_launch:
        b = np.flatnonzero(rec["front"][s0 + 1:s1] != rec["front"][s0:s1 - 1])
        two_fronts += int((b // chunk == (b + 1) // chunk).sum())
    return dict(records=len(got), chunk=chunk, ne=rec["ne"], na=rec["na"], n=rec["n"], per_col=per_col, rows_max=rows_max,
                empty_then_full=int(((rec["ne"][:-1] == 0) & (rec["ne"][1:] > 0)).sum()), za=rec["za"], zb=rec["zb"],
                idle_waves=int(((-nwaves) % 4).sum()), two_fronts=two_fronts, thick_many=thick_many, thick_long=thick_long)


@pytest.mark.parametrize("name", list(cases()))
def test_records_are_the_panel_segments_of_the_formed_fronts_in_launch_order(name):
    sh = analysed(name)
    print(name, {k: (v if np.isscalar(v) else (int(np.min(v)), int(np.max(v)))) for k, v in sh.items()})
    assert sh["records"] > 0


def test_the_inputs_contain_the_shapes_the_kernel_has_a_path_for():
    sh = {name: analysed(name) for name in cases()}
    chunk = sh["ba8"]["chunk"]
    assert chunk >= 4                                                  # fewer records per wave and there is nothing to fetch ahead across
    a = sh["ba8"]                       # one segment per column: a chunk is all cross-column; both sides of the 8-entry batch; the thick path; empty segments
    assert (a["per_col"] == 1).all()
    assert (a["ne"] == EG_EB).any() and (a["ne"] == EG_EB + 1).any() and (a["ne"] == 0).any() and a["ne"].max() == EG_EB + 1
    assert a["rows_max"].max() > 256 and a["thick_many"] > 0 and a["thick_long"] > 0      # the thick path, both moves of its cursor
    assert a["na"].max() > 32 and a["na"].max() <= 128 and (a["za"] > 0).any() and (a["zb"] > 0).any()
    b = sh["ba8-cap256"]                # up to 3 segments per column: first and last differ; an empty segment directly followed by a non-empty one
    assert b["per_col"].max() == 3 and (b["ne"] == 0).any() and b["empty_then_full"] > 0 and (b["na"] == 0).any()
    c = sh["ba8-cap64"]                 # long columns, tails of every length
    assert c["per_col"].max() >= 8 and set(range(1, 65)) <= set(c["n"].tolist())
    d = sh["stair25-cap3"]              # many segments per column, rows per segment below the 64 lanes, mostly empty
    assert d["per_col"].max() > 64 and d["n"].max() <= 3 and d["na"].max() <= 3 and (d["ne"] == 0).sum() > d["records"] // 2
    # across the inputs: a list that is no multiple of the chunk, launches whose last workgroup has fewer chunks than waves (waves with nothing to do),
    # chunks that span two fronts; no list longer than eg_put_formed's registers hold (its walk beyond them is the parent kernel's, textually)
    assert any(s["records"] % chunk for s in sh.values())
    assert all(s["idle_waves"] > 0 for s in sh.values())
    assert all(s["two_fronts"] > 0 for s in sh.values())
    assert max(s["na"].max() for s in sh.values()) <= 128


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def one_handle(A, kw):
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=0, **kw))
    try:
        m, n = kkt.m, kkt.n
        for seed in (0, 1, 2):
            th, rp, rd, xp, xd = step_data(m, n, seed)
            tk.update(kkt, th, rp, rd)
        dx = np.zeros(n); dy = np.zeros(m)
        tk.solve(dx, dy, kkt, xp, xd)
        return [kkt.factor_panels().copy(), dx, dy], kkt.symbolic("ea_seg_rec").size, int((kkt.symbolic("ea_form") != 0).sum()), stored_mask(kkt)
    finally:
        kkt.close()


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poison"])
@pytest.mark.parametrize("name", list(cases()))
def test_gpu_factor_and_solve_over_the_list_equal_the_task_driven_ones_bitwise(name, poison):
    A, kw, cap = cases()[name]
    res, mask = {}, {}
    for seglist in (0, 1):
        with seg_knobs(seglist, cap, poison):
            res[seglist], nrec, nform, mask[seglist] = one_handle(A, kw)
        assert nform > 0 and (nrec > 0) == (seglist == 1)
    assert all(np.isfinite(x).all() for x in res[1][1:3])             # (dx, dy)
    assert np.array_equal(mask[0], mask[1])
    if poison:
        assert same(res[1], res[0]), name                             # the whole factor storage (what no kernel writes holds the poison) and the solve
    # every stored double of every panel, padding rows included, and the solve (without the poison the doubles between panels are the allocation's)
    assert same([res[1][0][mask[1]]] + res[1][1:], [res[0][0][mask[0]]] + res[0][1:]), name


@pytest.mark.gpu
def test_gpu_a_skipped_block_is_passed_over_record_by_record():
    """three blocks in one launch, the middle one skipped: chunks of the list span a skipped and a live front"""
    from test_block_skip import pk_len
    A, rb = diag3()
    m, n = A.shape
    out = {}
    for seglist in (0, 1):
        with seg_knobs(seglist):
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
            if seglist:
                rec, launch = kkt.symbolic("ea_seg_rec").reshape(-1, len(FIELDS)), kkt.symbolic("ea_seg_launch").reshape(-1, 3)
                chunk = int(kkt.symbolic("ea_seg_chunk")[0])
                mixed = 0
                for _first, s0, s1 in launch:
                    skipped = fu[rec[s0:s1, 0]] == 1
                    b = np.flatnonzero(skipped[1:] != skipped[:-1])
                    mixed += int((b // chunk == (b + 1) // chunk).sum())
                assert mixed > 0                                  # a wave meets records of a skipped and of a live front in one chunk
            else:
                assert kkt.symbolic("ea_seg_rec").size == 0
            idx = [np.concatenate([np.arange(loff[s], loff[s] + pk_len(int(lda[s]), int(ns[s]))) for s in np.flatnonzero(fu == u)]) for u in range(3)]
            assert np.array_equal(F1[idx[1]], F0[idx[1]]), "the skipped block's panels were touched"
            assert not np.array_equal(F1[idx[0]], F0[idx[0]]) and not np.array_equal(F1[idx[2]], F0[idx[2]])
            mask = stored_mask(kkt)
            out[seglist] = [F0[mask], F1[mask]]                   # (the doubles between panels are the allocation's)
        finally:
            kkt.close()
    assert same(out[1], out[0])
