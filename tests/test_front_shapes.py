"""Front-shape sweep: elimination trees PLANTED so that a front sits on either side of every cut at which schedule.cpp hands a front to another
kernel (tlpk_host.hpp: SMALL_NS = 16, SMALL_ROWS = 256, TRSM_THIN_W = 32, NB_IN = 64, NB_OUT = 256, TILE = SOLVE_NB = 128, 64-row trsm strips,
LDA_PAD_MIN_F = 64, split-K from K = 512, the dependency-driven launch from ns = 769), checked with the criterion of tests/test_backward_error.py:
componentwise backward error against long double, omega_hard <= 1 and omega_unit <= 8 max(restatement's, 1).  The other GPU tests of these kernels
feed random sparse matrices, whose front shapes are whatever the ordering and the supernode detection make of them.

The recipe is lp_generators.planted_tree: with natural ordering and relax=False the analysed fronts are exactly the planted (ns, f, nchild) --
asserted on the CPU before anything runs on a GPU.  An input is a SPINE (a chain of fronts from the root down: front k of a spine has
f_k = ns_k + f_(k-1) - 1 rows, so a spine of a few narrow fronts offers its leaves every number of rows below one likes: f_k - 1) with LEAVES under
its fronts, plus whole further trees where a root shape is needed.  Every input has at most 1100 rows: the long-double residual covers every row.

CPU: the planted shapes; the shapes the sweep has to contain; the launch kinds; small fronts alone and merged; the kernel class of every front;
and the three legs of tests/test_backward_error.py per input and regime.  GPU (-m gpu): the device leg per input and regime, the mid one factorising
its data over the ones factor in NaN-poisoned storage; a pair of right-hand sides.  The table of a run on an MI355X is profiles/front_shape_sweep.txt."""
import copy

import numpy as np
import pytest

import tulip_jl_amd as tk
from backward_error import LD, Allowances, System, solve_stats
from emulate import LK, panels_to_dense_L
from helpers import DevBuf, ipm_like_data
from lp_generators import planted_tree
from test_backward_error import RATIO, SEED, Problem, _dense, device_leg, emulator_leg, mutation_leg

KIND = {v: k for k, v in LK.items()}
PLANT_SEED = 7


def tree(spine, leaves, more=()):
    """Postorder (ns, parent) list of: a spine (ns from the root down), leaves (ns, k) under spine front k, and `more` = further whole trees,
    each again (spine, leaves)."""
    nodes, at = [], {}
    for k in range(len(spine) - 1, -1, -1):
        nodes += [[ns, k] for ns, kk in leaves if kk == k]
        at[k] = len(nodes)
        nodes.append([spine[k], k - 1])
    out = [(ns, at[p] if p >= 0 else -1) for ns, p in nodes]
    for sp_, lv_ in more:
        out += [(ns, p + len(out) if p >= 0 else -1) for ns, p in tree(sp_, lv_)]
    return out


# name -> (spine, leaves, further trees).  In the comments: rb = rows below a front = f - ns; a leaf under spine front k has rb = f_k - 1.
TREES = {
    # spine f = 2, 16, 17, 18: ns = 257 (one block column + ONE column) over rb = 1, 15, 16, 17; ns = 16 | 17 over one row
    "x257_rb1_17": ([2, 15, 2, 2], [(257, 0), (257, 1), (257, 2), (257, 3), (16, 0), (17, 0)], ()),
    # spine f = 64, 65, 66 under a 64-column root: the 64-row trsm strip, f = 64 | 65 ... for ns = 257, 64, 16 | 17
    "rb63_65": ([64, 2, 2], [(257, 0), (257, 1), (257, 2), (64, 0), (64, 1), (64, 2), (16, 0), (17, 0), (16, 1)], ()),
    # spine f = 65, 128, 129, 130 (root 65, an interior 64-column front): the 128-row tile and solve block
    "rb127_129": ([65, 64, 2, 2], [(257, 1), (257, 2), (257, 3), (64, 1), (64, 2), (64, 3)], ()),
    # spine f = 256, 257, 258 under a 256-column root: SMALL_ROWS = 256 from both sides for ns = 16 (17 has no such cut: the control)
    "rb255_257": ([256, 2, 2], [(257, 0), (257, 1), (257, 2), (16, 0), (17, 0), (16, 1), (17, 1)], ()),
    # root 257, spine f = 257, 258, 259: every narrow pivot width over MORE than 256 rows (rb = 257 or 258); 64 over 256 | 257
    "tall": ([257, 2, 2], [(1, 2), (2, 2), (15, 2), (31, 2), (32, 2), (33, 2), (63, 2), (65, 2), (16, 1), (17, 1), (64, 1), (64, 0), (127, 1), (128, 1), (129, 1)], ()),
    # a ladder f = 16, 17, 18, 64, 65, 66, 128, 129, 130, 256 under a 16-column root: ns = 16 | 17 over every rb cut, 64 over 15 .. 17 and 255,
    # and the narrow pivot widths over FEWER than 64 rows
    "ladder": ([16, 2, 2, 47, 2, 2, 63, 2, 2, 127],
               [(16, 0), (17, 0), (16, 1), (17, 1), (16, 2), (17, 2), (17, 4), (16, 5), (17, 5), (16, 6), (17, 6), (16, 7), (17, 7), (16, 8), (17, 8),
                (64, 0), (64, 1), (64, 2), (64, 9), (1, 0), (2, 0), (15, 0), (31, 1), (32, 1), (33, 1), (63, 2), (65, 2)], ()),
    # spine f = 47, 48, 49, 50: f = 63, 64, 65 (LDA_PAD_MIN_F) reached from ns = 16 AND from ns = 17; the wide pivot blocks over 46 rows
    "f63_65": ([47, 2, 2, 2], [(17, 0), (16, 1), (17, 1), (16, 2), (17, 2), (16, 3), (127, 0), (128, 0), (129, 0), (255, 0), (256, 0)], ()),
    # interior fronts 16, 17, 32, 33, 65, 129 under a 17-column root; 16 has ONE child; the children of 32 straddle 15 | 17, those of 65 straddle
    # 64 | 65; 255 | 256 over 302 rows; two more trees: 64 over ONE row, and an isolated 1 x 1 root
    "interior": ([17, 16, 17, 32, 33, 65, 129], [(255, 6), (256, 6), (15, 3), (17, 3), (64, 5), (65, 5)], (([2], [(64, 0)]), ([1], []))),
    # interior 257 and 256 with one child each; a 513-column leaf (two block columns + one column; K = 512: split-K) over 512 rows
    "ns513": ([2, 257, 256], [(513, 2)], ()),
    "ns511_512": ([17, 33], [(511, 1), (512, 1)], ()),
    "ns768": ([256], [(768, 0)], ()),
    "ns769": ([257], [(769, 0)], ()),                 # the dependency-driven launch
    # a leaf level of small fronts only: k_fwd_small / k_bwd_small launched by themselves
    "small_only": ([70], [(15, 0), (16, 0), (1, 0), (2, 0)], ()),
}


def _planted(name):
    return lambda: (planted_tree(tree(*TREES[name]), PLANT_SEED)[0], dict(relax=False, ordering="natural"))


# the dense backend at the same criterion: the tile edge and the K-slab tail of the SYRK (m around 128, n around 16), one block column + 1
DENSE_SHAPES = [(m, n) for m in (127, 128, 129) for n in (15, 16, 17)] + [(257, 33)]
INPUTS = {name: ("k1", "sparse", _planted(name)) for name in TREES}
INPUTS.update({f"dense_{m}x{n}": ("k1", "dense", _dense(m, n)) for m, n in DENSE_SHAPES})
# Regime "late" (theta over 16 decades, 5 % exact zeros, regularisations sqrt(eps)) only where the restatement factorises it -- chosen on the CPU:
# every planted tree (with the values of PLANT_SEED); none of the dense inputs, whose A D A' has rank n < m and leaves the rest to a regularisation
# of sqrt(eps): the restatement meets a negative pivot between column 16 and column 38 on each of the ten.
LATE = list(TREES)
TREE_COMBOS = [(name, reg) for name in TREES for reg in ("ones", "mid", "late")]
COMBOS = TREE_COMBOS + [(f"dense_{m}x{n}", reg) for m, n in DENSE_SHAPES for reg in ("ones", "mid")]      # (the trees first: a prefix, see the mutation leg)
assert set(COMBOS) == {(name, reg) for name in INPUTS for reg in ("ones", "mid")} | {(name, "late") for name in LATE}
IDS = [f"{a}-{b}" for a, b in COMBOS]

_problems = {}


def problem(name, regime):
    """The mid problems are kept (the GPU legs of the second half of the file use them again); of the others the last one."""
    key = (name, regime)
    if key not in _problems:
        for k in [k for k in _problems if k[1] != "mid"]:
            del _problems[k]
        _problems[key] = Problem(name, regime, INPUTS)
    return _problems[key]


@pytest.fixture(scope="module", params=COMBOS, ids=IDS)
def pb(request):
    return problem(*request.param)


@pytest.fixture(scope="module")
def handles():
    """name -> (planted shapes, analysed CPU handle) of the sparse inputs"""
    out = {}
    for name in TREES:
        A, shapes = planted_tree(tree(*TREES[name]), PLANT_SEED)
        out[name] = (shapes, tk.setup(A, tk.K1(), tk.Backend(device=-1, relax=False, ordering="natural")))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the inputs are what they claim to be
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_analysed_fronts_are_the_planted_ones(handles):
    for name, (shapes, kkt) in handles.items():
        g = kkt.symbolic
        got = sorted(zip(g("front_ns").tolist(), g("front_f").tolist(), g("front_nchild").tolist()))
        assert got == sorted(shapes), name
        assert kkt.m <= 1100, name


def test_the_sweep_holds_every_shape_it_is_for():
    """The shape lists of the sweep, against the union of the planted (ns, rows below, nchild, children's ns)."""
    fronts = []
    for name in TREES:
        nodes = tree(*TREES[name])
        _, shapes = planted_tree(nodes, PLANT_SEED)
        kids = [[nodes[c][0] for c in range(len(nodes)) if nodes[c][1] == q] for q in range(len(nodes))]
        fronts += [(ns, f - ns, nch, tuple(sorted(kids[q])), nodes[q][1] < 0) for q, (ns, f, nch) in enumerate(shapes)]
    leaves = {(ns, rb) for ns, rb, nch, _, _ in fronts if nch == 0}
    for ns in (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257):      # pivot columns: over a few rows and over many
        assert any(a == ns and 0 < rb < 64 for a, rb in leaves) and any(a == ns and rb > 256 for a, rb in leaves), ns
    for ns in (511, 512, 513, 768, 769):
        assert any(a == ns and rb > 0 for a, rb in leaves), ns
    anyf = {(ns, rb) for ns, rb, *_ in fronts}
    for ns in (16, 17, 64, 257):                                                              # rows below
        for rb in (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257):
            assert (ns, rb) in anyf, (ns, rb)
    for f in (63, 64, 65):                                                                    # LDA_PAD_MIN_F from both sides of SMALL_NS
        assert (16, f - 16) in anyf and (17, f - 17) in anyf, f
    interior = [(ns, nch, kids) for ns, rb, nch, kids, root in fronts if nch > 0 and rb > 0]
    for ns in (16, 17, 32, 33, 64, 65, 129, 256, 257):
        assert any(a == ns for a, _, _ in interior), ns
    assert any(nch == 1 for _, nch, _ in interior)
    assert any({15, 17} <= set(kids) for _, _, kids in interior) and any({64, 65} <= set(kids) for _, _, kids in interior)
    roots = {ns for ns, rb, nch, kids, root in fronts if root}
    assert all(rb == 0 for ns, rb, nch, kids, root in fronts if root) and {1, 16, 17, 64, 65, 256, 257} <= roots


# The launch kinds of tests/emulate.py that no input has to reach: the markers, and the kinds the default knobs never emit.  Fixed.
EXEMPT = {"SIDE_FORK", "SIDE_JOIN", "WAIT_UPPER", "ALLREDUCE", "UPDATE_T64", "FRONT_ASSEMBLE", "FWD_DIAG", "FWD_UPDATE", "BWD_UPDATE", "BWD_DIAG"}


def launch_kinds(kkt):
    return {KIND[int(k)] for w in ("factor_launches", "fwd_launches", "bwd_launches") for k in kkt.symbolic(w).reshape(-1, 3)[:, 0]}


def missing_launch_kinds(handles, without=()):
    reached = set().union(*(launch_kinds(kkt) for name, (_, kkt) in handles.items() if name not in without))
    return set(LK) - EXEMPT - reached


def test_every_launch_kind_is_reached(handles):
    assert missing_launch_kinds(handles) == set()
    assert missing_launch_kinds(handles, without=["ns769"]) == {"CHAIN"}          # (the test has teeth: ns769 is the only carrier of the chain)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: which kernel a front gets (schedule.cpp: potrf_launches, trsm_launches, is_small, chain_rule)
# ---------------------------------------------------------------------------------------------------------------------------------
# A front's pivot columns are cut into block columns of 256 (the last: what is left).  Width of a block column -> potrf kernel, trsm kernel, rows per
# trsm task (tasks END on multiples of that many rows of the front).
WIDTH_RULES = [
    ((1, 32), "POTRF", "TRSM_THIN", 256),
    ((33, 64), "POTRF", "TRSM", 64),
    ((65, 256), "POTRF_WIDE", "TRSM", 64),
]
# (ns, rows below) -> what overrides the width rules in the factorisation, and the solve kernels
FRONT_RULES = [
    ((1, 16), (0, 256), "POTRF_SMALL", "SMALL"),              # potrf: one wave per front; k_fwd_small / k_bwd_small
    ((1, 16), (257, 10 ** 9), "POTRF_SMALL", "SWEEP"),        # thin but tall: the sweeps
    ((17, 768), (0, 10 ** 9), None, "SWEEP"),
    ((769, 10 ** 9), (0, 10 ** 9), "CHAIN", "SWEEP"),         # potrf and trsm as items of k_chain, 64-row strips for every width
]
# per sparse input: fronts in POTRF_SMALL, block columns in POTRF, in POTRF_WIDE, in TRSM_THIN, in TRSM, fronts in CHAIN, fronts in the small-front
# solve kernels, fronts in the sweeps.  Written down from TREES with the rules above: a planted ns moved across a cut changes a row.
CLASS_COUNTS = {
    "x257_rb1_17": (5, 5, 4, 9, 4, 0, 5, 5),          # e.g.: spine 2, 15, 2, 2 and the leaf 16 small; the last column of four 257s and the leaf 17 in POTRF
    "rb63_65": (4, 8, 3, 8, 6, 0, 4, 8),
    "rb127_129": (2, 7, 4, 5, 7, 0, 2, 8),
    "rb255_257": (4, 5, 4, 9, 3, 0, 4, 6),            # 16 over 256 rows: small solve; 16 over 257 rows: the sweep
    "tall": (6, 8, 5, 9, 9, 0, 1, 17),                # 1, 2, 15, 16 over 257 / 258 rows: POTRF_SMALL, but the sweep
    "ladder": (17, 18, 2, 26, 10, 0, 17, 20),
    "f63_65": (6, 4, 5, 9, 5, 0, 6, 9),
    "interior": (3, 7, 5, 5, 8, 0, 3, 12),
    "ns513": (1, 2, 4, 2, 4, 0, 1, 3),
    "ns511_512": (0, 2, 4, 0, 5, 0, 0, 4),
    "ns768": (0, 0, 4, 0, 3, 0, 0, 2),
    "ns769": (0, 1, 1, 0, 1, 1, 0, 2),                # the leaf: three block columns, all in the chain
    "small_only": (4, 0, 1, 4, 0, 0, 4, 1),
}


def rule(table, *key):
    hit = [row[len(key):] for row in table if all(lo <= v <= hi for v, (lo, hi) in zip(key, row))]
    assert len(hit) == 1, key
    return hit[0]


def classes_of(kkt):
    """From the exported launches and task lists: (front, k0) -> potrf kind; (front, k0) -> (trsm kind, tasks); front -> solve class per direction;
    and per sweep launch whether it carries merged small-front items."""
    g = kkt.symbolic
    potrf_t, trsm_t, chain = g("potrf_tasks").reshape(-1, 4), g("trsm_tasks").reshape(-1, 6), g("chain_items").reshape(-1, 12)
    potrf, trsm = {}, {}

    def add_trsm(t, kind):
        old = trsm.setdefault((int(t[0]), int(t[1])), [kind, 0])
        assert old[0] == kind
        old[1] += 1
    for kind, first, count in g("factor_launches").reshape(-1, 3).tolist():
        kind = KIND[kind]
        if kind == "POTRF_SMALL":
            for t in potrf_t[first: first + 4 * count]:
                if t[0] >= 0:
                    assert (int(t[0]), int(t[1])) not in potrf
                    potrf[(int(t[0]), int(t[1]))] = kind
        elif kind in ("POTRF", "POTRF_WIDE"):
            for t in potrf_t[first: first + count]:
                assert (int(t[0]), int(t[1])) not in potrf
                potrf[(int(t[0]), int(t[1]))] = kind
        elif kind in ("TRSM", "TRSM_THIN"):
            for t in trsm_t[first: first + count]:
                add_trsm(t, kind)
        elif kind == "CHAIN":
            for it in chain[first: first + count]:
                if it[0] == 1:
                    t = potrf_t[it[1]]
                    potrf[(int(t[0]), int(t[1]))] = "CHAIN"
                elif it[0] == 2:
                    add_trsm(trsm_t[it[1]], "CHAIN")
    solve, merged = {}, {}
    for way, small_kind, sweep_kind in (("fwd", "FWD_SMALL", "FWD_SWEEP"), ("bwd", "BWD_SMALL", "BWD_SWEEP")):
        small_t, sweep_t = g(way + "_small_tasks").reshape(-1, 6), g(way + "_sweep_tasks").reshape(-1, 6)
        cls, flags = {}, []
        for kind, first, count in g(way + "_launches").reshape(-1, 3).tolist():
            if KIND[kind] == small_kind:
                cls.update({int(t[0]): "SMALL" for t in small_t[first: first + 4 * count] if t[0] >= 0})
            elif KIND[kind] == sweep_kind:
                items = sweep_t[first: first + count]
                is_small_item = (items[:, 4] == 2) if way == "fwd" else (items[:, 5] == -2)
                flags.append(bool(is_small_item.any()))
                for it in items[is_small_item]:
                    cls.update({int(t[0]): "SMALL" for t in small_t[4 * it[1]: 4 * it[1] + 4] if t[0] >= 0})
                for it in items[~is_small_item]:
                    assert cls.setdefault(int(it[0]), "SWEEP") == "SWEEP"
        solve[way], merged[way] = cls, flags
    return potrf, trsm, solve, merged


def test_every_front_goes_to_the_kernels_its_shape_asks_for(handles):
    for name, (shapes, kkt) in handles.items():
        potrf, trsm, solve, _ = classes_of(kkt)
        g = kkt.symbolic
        want_potrf, want_trsm, want_solve = {}, {}, {}
        for s, (ns, f) in enumerate(zip(g("front_ns").tolist(), g("front_f").tolist())):
            if g("front_single")[s]:                                     # an isolated 1 x 1 root: k_single_factor / k_single_solve, in no task list
                assert (ns, f) == (1, 1)
                continue
            over, cls = rule(FRONT_RULES, ns, f - ns)
            want_solve[s] = cls
            for k0 in range(0, ns, 256):
                w = min(256, ns - k0)
                pk, tk_, step = rule(WIDTH_RULES, w)
                want_potrf[(s, k0)] = over or pk
                if over == "CHAIN":
                    tk_, step = "CHAIN", 64
                r0, ntask = k0 + w, 0
                while r0 < f:
                    r0, ntask = min(f, (r0 // step + 1) * step), ntask + 1
                if ntask:
                    want_trsm[(s, k0)] = [tk_, ntask]
        assert potrf == want_potrf, name
        assert trsm == want_trsm, name
        assert solve["fwd"] == want_solve and solve["bwd"] == want_solve, name
        count = lambda d, v: sum(1 for x in d.values() if (x[0] if isinstance(x, list) else x) == v)      # noqa: E731
        got = (count(potrf, "POTRF_SMALL"), count(potrf, "POTRF"), count(potrf, "POTRF_WIDE"), count(trsm, "TRSM_THIN"), count(trsm, "TRSM"),
               len({s for (s, _), v in potrf.items() if v == "CHAIN"}), count(solve["fwd"], "SMALL"), count(solve["fwd"], "SWEEP"))
        assert got == CLASS_COUNTS[name], (name, got)


def test_small_fronts_ride_in_a_sweep_and_run_alone(handles):
    """k_fwd_small / k_bwd_small as launches of their own (a level of small fronts only) and as items of the sweep's launch (a level that has both);
    sweep launches with and without such items."""
    flags = {"fwd": [], "bwd": []}
    for name, (_, kkt) in handles.items():
        merged = classes_of(kkt)[3]
        for way in flags:
            flags[way] += merged[way]
    assert all(True in v and False in v for v in flags.values())
    alone = launch_kinds(handles["small_only"][1])
    assert {"FWD_SMALL", "BWD_SMALL"} <= alone
    potrf, trsm, solve, merged = classes_of(handles["small_only"][1])
    assert merged == {"fwd": [False], "bwd": [False]}                # the root's sweep; the leaf level has no sweep to ride in
    assert True in classes_of(handles["ladder"][1])[3]["fwd"] and True in classes_of(handles["ladder"][1])[3]["bwd"]


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the three legs of tests/test_backward_error.py
# ---------------------------------------------------------------------------------------------------------------------------------
def test_restatement_is_inside_the_bound(pb):
    pb.assert_good_input()


def test_emulated_schedule_is_inside_the_bound(pb):
    emulator_leg(pb)


@pytest.mark.parametrize("pb", TREE_COMBOS, ids=IDS[:len(TREE_COMBOS)], indirect=True)
def test_mutation_one_small_entry_passes_the_normwise_criteria_and_fails_the_bound(pb):
    """On the planted trees.  The dense shapes are left to the bounds: their K^ = A D A' + Rd has rank n << m plus a small multiple of I, every row of
    it is full, and the allowance of a row of the SOLVE then sums over all m entries of w -- in regime mid w_k (1 + 1e-10) moves omega_hard of the solve from
    1.6e-05 to 0.46 on dense_257x33, to 0.71, 0.91, 0.73 on 127x15, 127x16, 128x15 and to 1.07 .. 2.3 on the other six (regime ones: 11 .. 23; the
    factor's omega_hard goes above 8 on all twenty).  The leg is a statement about the checker, and on these inputs it would state a coin toss."""
    mutation_leg(pb)


def test_late_data_is_used_where_the_restatement_factorises_it():
    """One of the inputs left out of LATE: the restatement meets a negative pivot there, so the regime is no test input (and would be a FAILURE of
    test_restatement_is_inside_the_bound, not a skip, were it listed)."""
    assert "dense_257x33" not in LATE
    p = Problem("dense_257x33", "late", INPUTS)
    assert "error" in p.stats and p.L is None


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
MID = [name for name in INPUTS]


@pytest.mark.gpu
def test_device_factor_and_solves_are_inside_the_bound(pb, monkeypatch):
    """The device leg of tests/test_backward_error.py.  The leg of regime mid is the one with stale storage: TLPK_POISON=1 (the factor storage starts as
    NaNs), the ones data factorised first, then the mid data on the same handle -- a zero-fill that misses an edge, or an update-matrix buffer that
    keeps what the first factorisation left there, shows in the second factor."""
    if pb.regime != "mid":
        return device_leg(pb)
    monkeypatch.setenv("TLPK_POISON", "1")
    m, n = pb.A.shape
    device_leg(pb, who="device+stale", first=ipm_like_data(m, n, SEED, "ones")[:3])


def with_rhs(system, xp, xd):
    """The K1 system with another right-hand side (xi_p, xi_d): rhs = xi_p + A D xi_d and its allowances, as System forms them.  K2: rhs =
    [xi_d; xi_p], a permutation of the caller's -- no arithmetic, no allowance."""
    out = copy.copy(system)
    if system.kind == "k2":
        out.data = system.data[:3] + (xp, xd)
        out.rhs = np.concatenate([xd, xp]).astype(LD)[system.perm]
        out.rhs_hard = out.rhs_unit = np.zeros(system.N)
        return out
    assert system.kind == "k1"
    A, D = system.A, system.D
    absA = abs(A)
    q = np.asarray((absA != 0).sum(axis=1)).ravel().astype(np.float64)
    ra = np.abs(xp) + np.asarray(absA @ (D * np.abs(xd))).ravel()
    out.data = system.data[:3] + (xp, xd)
    out.rhs = (xp.astype(LD) + System._matvec(A, D.astype(LD) * xd.astype(LD)))[system.perm]
    out.rhs_hard = ((q + 3 + q / 2048.0) * ra)[system.perm]
    out.rhs_unit = ra[system.perm]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", MID)
def test_device_pair_of_right_hand_sides(name):
    """tlpk_solve2_device: both solutions bit for bit those of two single solves, and both inside the solve bound of the device's own factor."""
    pb = problem(name, "mid")
    pb.assert_good_input()
    backend = tk.DenseBackend(device=0) if INPUTS[name][1] == "dense" else tk.Backend(device=0, relax=False, ordering="natural")
    kkt = tk.setup(pb.A, tk.K1(), backend)
    th, rp, rd, xp, xd = pb.data
    m, n = pb.A.shape
    rhs = [(xp, xd), (xp[::-1].copy(), xd[::-1].copy())]
    tk.update(kkt, th, rp, rd)
    single = []
    for p, d in rhs:
        dx = np.zeros(n); dy = np.zeros(m)
        tk.solve(dx, dy, kkt, p, d)
        single.append((dx, dy))
    d = [DevBuf(v) for v in (rhs[0][0], rhs[0][1], rhs[1][0], rhs[1][1])]
    o = [DevBuf(sz, np.nan) for sz in (n, m, n, m)]
    kkt.solve2_device(o[0].ptr, o[1].ptr, d[0].ptr, d[1].ptr, o[2].ptr, o[3].ptr, d[2].ptr, d[3].ptr)
    pair = [(o[0].get(), o[1].get()), (o[2].get(), o[3].get())]
    L = np.tril(panels_to_dense_L(kkt, kkt.factor_panels()))
    kkt.close()
    for (dx, dy), (dx1, dy1) in zip(single, pair):
        assert dx.tobytes() == dx1.tobytes() and dy.tobytes() == dy1.tobytes()
    allow = Allowances(pb.system, L, pb.blocks)
    ref = pb.stats["solve"]["unit"]
    for k, (sysk, (dx, dy)) in enumerate(zip((pb.system, with_rhs(pb.system, *rhs[1])), pair)):
        allow.system = sysk
        v = solve_stats(allow, sysk.permuted(dx, dy))
        print(f"BE {name:15s} mid   pair rhs {k}  N={sysk.N:5d} | solve hard={v['hard']:.3e} unit={v['unit']:.3e}")
        assert v["hard"] <= 1.0, f"{name} rhs {k}: omega_hard = {v['hard']:.3e} at {v['at']}"
        assert v["unit"] <= RATIO * max(ref, 1.0), f"{name} rhs {k}: omega_unit = {v['unit']:.3e}, the restatement's {ref:.3e}"
