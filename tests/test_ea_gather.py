"""Extend-add by parent column (k_ea_gather, TLPK_EA_GATHER).

CPU (analyse-only handles): the exported per-column index is exactly the inverse of `rel` -- every (parent column, child, child column q) once per
segment of the column it has rows in (a column of at most TLPK_EA_GATHER_CAP rows is one segment: once, with rs_c - q rows), the contributors of a segment
in the order of the parent's child list --, each entry carries the offsets and the row count the kernel reads, the pieces of a child column tile its rows
q .. rs_c, no segment is longer than the LDS slice of its launch, and the hashed schedule arrays do not depend on the knob.

GPU: the factor panels and a solve of the gathered form against the plain kernel's, bit for bit, after three updates on one handle (both U buffers are
reused), with and without TLPK_POISON=1.  The minimum child count is 1, so every parent front is gathered."""
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
from helpers import block_angular, ipm_like_data, load_golden  # noqa: E402

LK_EXTEND_ADD = 0
UBUF_BIT = 62
KNOBS = ("TLPK_EA_GATHER", "TLPK_EA_GATHER_MIN_CHILD", "TLPK_EA_GATHER_CAP", "TLPK_POISON")
HASHED = ["ea_tasks", "ea_tab", "rel", "factor_launches", "launch_meta", "zero_tasks", "zero_small", "update_tasks", "front_uoff", "front_loff"]


@contextlib.contextmanager
def knobs(gather, cap=None, poison=False):
    """the environment of ONE handle's creation (the knobs are read there): gather 0 = k_extend_add only, 1 = every parent front with a child"""
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ["TLPK_EA_GATHER"] = str(int(gather))
    os.environ["TLPK_EA_GATHER_MIN_CHILD"] = "1"
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


@functools.lru_cache(maxsize=None)
def ba8():
    return block_angular(nblocks=8, mk=700, nk=1400, m0=100, nnz_in=4, link_prob=0.5, seed=3)


@functools.lru_cache(maxsize=None)
def stair25():
    from tulip_jl_amd.problem import read_free_mps, standard_form
    return standard_form(read_free_mps(os.path.join(HERE, "golden", "stair25.mps"))).A


@functools.lru_cache(maxsize=None)
def gs2600():
    from workloads import general_sparse_lp
    return general_sparse_lp(2600)


def cpu_cases():
    A, rb = ba8()
    out = {"ba8": (A, tk.K1(), dict(row_block=rb), None), "ba8-cap256": (A, tk.K1(), dict(row_block=rb), 256),
           "ba8-k2": (A, tk.K2(), dict(row_block=rb), None), "ba8-rank1of2": (A, tk.K1(), dict(row_block=rb, rank=1, nranks=2), None),
           "stair25": (stair25(), tk.K1(), {}, None), "stair25-cap3": (stair25(), tk.K1(), {}, 3)}
    for g in load_golden():
        out[f"golden-{g['name']}"] = (g["A_csc"], tk.K1(), {}, None)
    return out


def expected_index(g, cap):
    """front -> column -> segment -> the list of (src, rel offset, rows, child) that `rel` defines, in the order k_extend_add applies them: the children in
    the order of the parent's child list; of child column q, rel[q] == tc, the rows [ra, rb) whose parent rows lie in [tc + p cap, tc + (p + 1) cap).
    Also checked here: the pieces of one (tc, child, q) follow each other without a gap from the diagonal q down to the last row rs_c."""
    f, ns, nchild, cptr, children = g("front_f"), g("front_ns"), g("front_nchild"), g("front_child_ptr"), g("children")
    reloff, uoff, ubuf, rel = g("front_reloff"), g("front_uoff"), g("front_ubuf"), g("rel")
    out = {}
    for s in range(len(f)):
        cols = [[[] for _ in range(-(-int(f[s] - tc) // cap))] for tc in range(int(f[s]))]
        for c in children[cptr[s]:cptr[s] + nchild[s]]:
            rsc = int(f[c] - ns[c])
            rl = rel[reloff[c]:reloff[c] + rsc]
            for q in range(rsc):
                tc = int(rl[q])
                cuts = np.searchsorted(rl, tc + cap * np.arange(len(cols[tc]) + 1))
                assert cuts[0] == q and cuts[-1] == rsc            # (rel is ascending: rows from the diagonal down, every row in some segment)
                for pc, (ra, rb) in enumerate(zip(cuts[:-1], cuts[1:])):
                    if rb > ra:
                        cols[tc][pc].append(((int(uoff[c]) + q * rsc + int(ra)) | (int(ubuf[c]) << UBUF_BIT), int(reloff[c]) + int(ra), int(rb - ra), int(c)))
        out[s] = cols
    return out


@pytest.mark.parametrize("name", list(cpu_cases()))
def test_index_is_the_inverse_of_rel_in_child_order(name):
    A, system, kw, cap = cpu_cases()[name]
    with knobs(1, cap):
        kkt = tk.setup(A, system, tk.Backend(device=-1, **kw))
    with knobs(0):
        plain = tk.setup(A, system, tk.Backend(device=-1, **kw))
    g = kkt.symbolic
    for w in HASHED:                                              # the knob moves nothing the schedule digest covers
        assert np.array_equal(g(w), plain.symbolic(w)), w
    for w in ("ea_gather_ent", "ea_gather_ptr", "ea_gather_col", "ea_gather_launches"):
        assert plain.symbolic(w).size == 0, w
    assert (plain.symbolic("ea_gather_base") == -1).all()
    base, col, ptr, ent = g("ea_gather_base"), g("ea_gather_col"), g("ea_gather_ptr"), g("ea_gather_ent").reshape(-1, 4)
    slice_cap = int(g("ea_gather_cap")[0])
    assert slice_cap == (cap if cap is not None else 1024)
    f, nchild, local, fa = g("front_f"), g("front_nchild"), g("front_local"), g("front_fa")
    want = expected_index(g, slice_cap)
    nseg = 0
    whole = 0
    for s in range(len(f)):
        selected = bool(local[s]) and nchild[s] >= 1 and not fa[s]
        assert (base[s] >= 0) == selected, s
        if not selected:
            continue
        cs = col[base[s]:base[s] + f[s] + 1]
        assert cs[0] == nseg                                      # the fronts' segments follow each other without gaps
        for tc in range(int(f[s])):
            assert cs[tc + 1] - cs[tc] == len(want[s][tc]) == -(-int(f[s] - tc) // slice_cap)      # no segment is longer than the slice
            for pc, exp in enumerate(want[s][tc]):
                seg = cs[tc] + pc
                got = [tuple(int(x) for x in e) for e in ent[ptr[seg]:ptr[seg + 1]]]
                assert got == exp, (s, tc, pc)                    # the triples once each, child order, the rows of the segment
            if len(want[s][tc]) == 1:
                whole += len(want[s][tc][0])
        nseg = int(cs[-1])
    assert (len(ptr) == nseg + 1 and ptr[0] == 0 and ptr[-1] == len(ent) and (np.diff(ptr) >= 0).all()) if nseg else len(ptr) == 0
    if name.startswith("ba8"):
        assert whole > 0                                          # columns of one segment: one entry per (column, child, q) with rs_c - q rows
    # the launches: the slice holds the longest segment of the launch, and the two task counts are what the kernels' rule gives
    tasks = g("ea_tasks").reshape(-1, 6)
    launches = {int(r[0]): r[1:] for r in g("ea_gather_launches").reshape(-1, 4)}
    seen = 0
    for kind, first, count in g("factor_launches").reshape(-1, 3):
        if kind != LK_EXTEND_ADD or count <= 0:
            continue
        n_gather = n_plain = longest = 0
        for front, j0, j1, _bidx, _br0, br1 in tasks[first:first + count]:
            gath = base[front] >= 0 and br1 == 0
            n_gather += gath; n_plain += not gath
            if gath:
                longest = max(longest, min(int(f[front] - j0), slice_cap))
        if n_gather:
            assert tuple(launches[int(first)]) == (n_gather, n_plain, longest) and longest <= slice_cap
            seen += 1
        else:
            assert int(first) not in launches
    assert seen == len(launches)
    if name == "ba8-cap256":
        # columns of exactly 256 rows (one segment) and of 257 rows (a second segment of one row), also among the update-matrix columns of a front with an odd ns
        ns = g("front_ns")
        assert any(base[s] >= 0 and f[s] >= 257 for s in range(len(f)))
        assert any(base[s] >= 0 and ns[s] % 2 == 1 and f[s] - ns[s] >= 257 for s in range(len(f)))


def test_auto_rule_takes_the_big_parents_only():
    """unset = auto: parents of at least 2048 rows with at least 16 children that hit them densely; ba8's fronts are smaller, so nothing is built"""
    A, rb = ba8()
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        kkt = tk.setup(A, tk.K1(), tk.Backend(device=-1, row_block=rb))
        assert kkt.symbolic("front_f").max() < 2048 and (kkt.symbolic("ea_gather_base") == -1).all() and kkt.symbolic("ea_gather_ent").size == 0
        # two blocks of the flagship shape (config C4): exactly the blocks' top fronts, not the root front (1000 rows) nor the fronts below
        from workloads import block_angular_lp
        B, rbb = block_angular_lp(2, 5000, 10000, 1000, 4, 0.5)
        big = tk.setup(B, tk.K1(), tk.Backend(device=-1, row_block=rbb))
        chosen = np.nonzero(big.symbolic("ea_gather_base") >= 0)[0]
        f, blk = big.symbolic("front_f"), big.symbolic("front_block")
        assert len(chosen) == 2 and (f[chosen] >= 2048).all() and sorted(blk[chosen]) == [0, 1] and big.symbolic("root_front")[0] not in chosen
        assert len(big.symbolic("ea_gather_launches")) > 0
    finally:
        os.environ.update({k: v for k, v in saved.items() if v is not None})


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def three_updates_and_a_solve(kkt):
    m, n = kkt.m, kkt.n
    for seed in (0, 1, 2):
        th, rp, rd, xp, xd = ipm_like_data(m, n, seed)
        tk.update(kkt, th, rp, rd)
    dx = np.zeros(n); dy = np.zeros(m)
    tk.solve(dx, dy, kkt, xp, xd)
    return [kkt.factor_panels().copy(), dx, dy]


def one_handle(A, system, kw):
    kkt = tk.setup(A, system, tk.Backend(device=0, **kw))
    try:
        return three_updates_and_a_solve(kkt), kkt.symbolic("ea_gather_launches").reshape(-1, 4)
    finally:
        kkt.close()


def sharded(A, kw):
    from test_set_values import sharded_step
    ks = [tk.setup(A, tk.K1(), tk.Backend(device=0, rank=r, nranks=2, **kw)) for r in range(2)]
    try:
        m, n = ks[0].m, ks[0].n
        for seed in (0, 1, 2):
            out = sharded_step(ks, ipm_like_data(m, n, seed))
        raw = [k.factor_panels().copy() for k in ks]
        return [np.concatenate(raw), out[1], out[2]] + out, np.concatenate([k.symbolic("ea_gather_launches").reshape(-1, 4) for k in ks])
    finally:
        for k in ks:
            k.close()


def gpu_cases():
    A, rb = ba8()
    out = {"ba8-k1": (A, tk.K1(), dict(row_block=rb), None), "ba8-k2": (A, tk.K2(), dict(row_block=rb), None),
           "ba8-ranks": (A, None, dict(row_block=rb), None), "ba8-cap256": (A, tk.K1(), dict(row_block=rb), 256),
           "gs2600": (None, tk.K1(), {}, None), "golden": (None, tk.K1(), {}, None)}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poison"])
@pytest.mark.parametrize("name", list(gpu_cases()))
def test_gpu_gathered_factor_and_solve_equal_the_plain_kernels_bitwise(name, poison):
    A, system, kw, cap = gpu_cases()[name]
    mats = [g["A_csc"] for g in load_golden()] if name == "golden" else [gs2600() if name == "gs2600" else A]
    gathered_launches = 0
    for M in mats:
        res = {}
        for form in (0, 1):
            with knobs(form, cap, poison):
                res[form], launches = sharded(M, kw) if system is None else one_handle(M, system, kw)
            if form == 0:
                assert len(launches) == 0
            else:
                gathered_launches += len(launches)
        assert all(np.isfinite(x).all() for x in res[0][1:3])         # (dx, dy)
        assert same(res[1], res[0]), name
    assert gathered_launches > 0 or name == "golden"                  # (the golden LPs are too small for a parent front to be certain)
    if name == "gs2600":
        with knobs(1):
            assert tk.setup(mats[0], system, tk.Backend(device=-1)).symbolic("front_f").max() >= 2048
