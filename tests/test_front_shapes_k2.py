"""Front-shape sweep of the SIGNED kernels: the sweep of tests/test_front_shapes.py with system = K2, on elimination trees planted with a
known SIGN PATTERN in every front.  K2 is served by the second instantiation of every factor kernel (template<bool SIGNED>), which multiplies by
the K columns' signs while staging the update's operand, applies the column signs at the trsm stores, forms 1 / (signed pivot) in the potrf kernels
and runs k_apply_signs between the sweeps.  A sign that is wrong in ONE column of a 256-wide block, or applied twice at a tail store, passes the
normwise K2 tests; here every front is checked componentwise against long double (tests/test_backward_error.py: omega_hard <= 1 and
omega_unit <= 8 max(restatement's, 1)).

The recipe is lp_generators.planted_tree_k2: a caller's permutation of the m + n nodes (ordering="user", relax=False) under which the analysed
fronts are exactly the planted (ns, f, nchild) AND sign strings -- read back from perm and asserted on the CPU before anything runs on a GPU.
The rows below a front are its ancestors' '+' rows: a front of p '+' offers its children p - 1 rows more than it has below itself, so the spines
below are written as patterns and the rows below follow from their '+' counts.  Every node brings a one-column helper front of sign - (transposed
trees: +) as a further leaf.  Every input has N = m + n <= 1100: the long-double residual covers every row.

CPU: planted = analysed; the shapes and sign patterns the sweep has to contain; the launch kinds; the kernel class of every front; the three legs
per input and regime; one wrong sign in the update step alone.  GPU (-m gpu): the device leg per input and regime, the mid one over the ones factor
in NaN-poisoned storage; a pair of right-hand sides.  The table of a run on an MI355X is profiles/front_shape_sweep_k2.txt."""
import numpy as np
import pytest

import tulip_jl_amd as tk
from backward_error import Allowances, dense_L_of_emulator, solve_stats
from emulate import Emulator, panels_to_dense_L
from helpers import DevBuf, ipm_like_data
from lp_generators import planted_tree_k2
from test_backward_error import RATIO, SEED, Problem, device_leg, emulator_leg, make_handle, mutation_leg
from test_front_shapes import FRONT_RULES, WIDTH_RULES, classes_of, missing_launch_kinds, rule, tree, with_rhs
from test_front_shapes import handles as k1_handles      # noqa: F401  (the K1 sweep's analysed handles: the launch kinds it reaches)

PLANT_SEED = 7
CUTS = (16, 32, 64, 128, 256, 512)           # the column cuts inside a pivot block: SMALL_NS, TRSM_THIN_W, NB_IN, TILE, NB_OUT, split-K


# ---------------------------------------------------------------------------------------------------------------------------------
# sign patterns.  All start with '+' (a transposed input exchanges the signs).  A flip AT b: pattern[b - 1] != pattern[b].
# ---------------------------------------------------------------------------------------------------------------------------------
def flips(ns, at):
    at, out, sign = set(at), [], "+"
    assert all(0 < b < ns for b in at)
    for k in range(ns):
        if k in at:
            sign = "-" if sign == "+" else "+"
        out.append(sign)
    return "".join(out)


def alt(ns):                 # fully alternating
    return flips(ns, range(1, ns))


def at_cuts(ns):             # a flip between columns c - 1 | c of every cut
    return flips(ns, [c for c in CUTS if c < ns])


def past_cuts(ns):           # a flip between columns c | c + 1 of every cut
    return flips(ns, [c + 1 for c in CUTS if c + 1 < ns])


def runs(ns, k):             # runs of k
    return flips(ns, range(k, ns, k))


def pm(ns):                  # '+' followed by all '-'
    return "+" + "-" * (ns - 1)


def lastm(ns):               # a single '-' as the last pivot column
    return "+" * (ns - 1) + "-"


def mixp(ns, p):             # ns columns of which p are '+': alternating from the first column, the surplus '+' last
    assert 1 <= ns - p <= p
    return "+-" * (ns - p) + "+" * (2 * p - ns)


S2 = "+-+"                   # the spine step: a front of two '+' offers its children ONE row more than it has below itself


# name -> (spine from the root down, leaves (pattern, k) under spine front k, further whole trees, transposed).  In the comments R = the rows
# below a child of the spine front = sum over the spine so far of ('+' count - 1).
TREES = {
    # R = 1, 15, 16, 17: ns = 257 over few rows with every pattern family; 16 | 17 alternating over one row; a single '-' last (the 16-front)
    "x257_rb1_17": ([S2, lastm(16), S2, S2], [(alt(257), 0), (at_cuts(257), 1), (past_cuts(257), 2), (runs(257, 64), 3), (alt(16), 0), (alt(17), 0)], (), False),
    # R = 63, 64, 65 under a 128-column alternating root: the 64-row trsm strip for ns = 257
    "x257_rb63_65": ([alt(128), S2, S2], [(pm(257), 0), (lastm(257), 1), (runs(257, 3), 2), (alt(64), 0), (at_cuts(64), 1), (alt(16), 1)], (), False),
    # R = 46 .. 49, 63, 64, 65: f = 63, 64, 65 (LDA_PAD_MIN_F) from ns = 16 AND from ns = 17; an interior 17 with three children; wide blocks over 46 rows
    "f63_65": ([mixp(64, 47), S2, S2, S2, mixp(17, 15), S2, S2],
               [(alt(17), 0), (alt(16), 1), (pm(17), 1), (runs(16, 3), 2), (at_cuts(17), 2), (runs(16, 7), 3), (alt(16), 4), (alt(17), 4), (runs(17, 2), 5),
                (runs(17, 4), 6), (lastm(16), 6), (past_cuts(64), 6), (at_cuts(127), 0), (past_cuts(128), 0), (at_cuts(129), 0), (at_cuts(255), 0),
                (at_cuts(32), 0), (at_cuts(33), 0)], (), False),
    # R = 127, 128, 129 under a 129-column root and an interior alternating 65 with three children: the 128-row tile and solve block
    "x257_rb127_129": ([mixp(129, 96), alt(65), S2, S2], [(at_cuts(257), 1), (alt(257), 2), (past_cuts(257), 3), (runs(64, 3), 1)], (), False),
    # R = 127, 128, 129 for 64, 16 | 17, under an interior 64 (flips at 16 and 32) with two children; two further trees: alternating roots 16 and 17
    "rb127_129": ([alt(129), at_cuts(64), mixp(17, 16), S2, S2, S2],
                  [(pm(17), 1), (pm(64), 3), (lastm(64), 4), (alt(64), 5), (alt(16), 3), (at_cuts(17), 3), (runs(16, 2), 4), (alt(17), 4), (pm(16), 5), (lastm(17), 5)],
                  (([alt(16)], []), ([alt(17)], [])), False),
    # R = 255, 256, 257 under a 258-column root: ns = 257 around SMALL_ROWS and the second solve block; 16 | 17 over 255, 16 over 256
    "x257_rb255_257": ([mixp(258, 256), S2, S2], [(runs(257, 64), 0), (at_cuts(257), 1), (alt(257), 2), (alt(16), 0), (alt(17), 0), (runs(16, 3), 1)], (), False),
    # an INTERIOR 257 (flips at every cut, two children) and an interior 129; R = 16, 191, 255, 256, 257; 64 over 255 .. 257; the narrow widths over 257 rows
    "tall_narrow": ([alt(33), at_cuts(257), alt(129), S2, S2],
                    [(alt(15), 1), (alt(64), 2), (past_cuts(64), 3), (runs(64, 16), 4), (alt(17), 3), (runs(16, 5), 4), (runs(17, 4), 4),
                     ("+-", 4), (runs(15, 4), 4), (at_cuts(31), 4), (past_cuts(32), 4), (at_cuts(33), 4), (at_cuts(63), 4), (past_cuts(65), 4), (past_cuts(127), 4)], (), False),
    # the wide widths over 257 rows
    "tall_wide": ([mixp(258, 256), S2, S2], [(at_cuts(128), 2), (past_cuts(129), 2), (past_cuts(255), 2), (at_cuts(256), 2)], (), False),
    # R = 1, 15, 16, 17 for ns = 64 and 16 | 17; the other widths over fewer than 64 rows; one more tree: a 257-column root by itself
    "ladder": ([S2, lastm(16), S2, S2],
               [(alt(64), 0), (pm(64), 1), (lastm(64), 2), (at_cuts(64), 3), (runs(16, 5), 1), (runs(17, 3), 1), (pm(16), 2), (alt(17), 2), (alt(16), 3), (runs(17, 4), 3),
                ("+-", 0), (alt(15), 1), (runs(31, 5), 2), (at_cuts(63), 2), (at_cuts(65), 3), (past_cuts(256), 1)], (([at_cuts(257)], []),), False),
    # split-K (K = 512): 513 = two block columns + ONE column, flips at 255 | 256 and 511 | 512; 511 with the flips one column later
    "ns511_513": ([alt(33)], [(at_cuts(513), 0), (past_cuts(511), 0)], (), False),
    # 512 = two full block columns, flips at 254 | 255 and 256 | 257, under an interior 65; one more tree: an alternating 257-column root by itself
    "ns512": ([S2, mixp(65, 33)], [(flips(512, [17, 33, 65, 129, 255, 257, 300]), 1), (alt(64), 1)], (([alt(257)], []),), False),
    # 768 = three block columns, flips at 512 | 513 and 513 | 514
    "ns768": ([alt(33)], [(flips(768, [16, 32, 64, 128, 256, 257, 400, 512, 513, 514, 700]), 0)], (), False),
    # the dependency-driven launch: a flip inside each block column and at 255 | 256 and 511 | 512
    "ns769": ([alt(129)], [(flips(769, [64, 128, 256, 300, 512, 600, 700]), 0)], (), False),
    # a small tree whose late data the restatement factorises: a 257-column leaf flipping every 64, 16 alternating, '+' followed by sixteen '-', 64 in
    # runs of 3, under an alternating 65-column root
    "mixed424": ([alt(65)], [(runs(257, 64), 0), (alt(16), 0), (pm(17), 0), (runs(64, 3), 0)], (), False),
    # TRANSPOSED (first pivot negative, over negative ancestors; the helpers are rows)
    "t_x257": ([S2, lastm(16), S2, S2], [(at_cuts(257), 1), (alt(257), 3), (alt(64), 2), (alt(16), 0), (alt(17), 3), (pm(33), 1), (past_cuts(129), 2), (lastm(65), 0)], (), True),
    "t_ns513": ([alt(65), alt(17)], [(at_cuts(513), 1), (runs(64, 3), 0), (alt(16), 0)], (), True),
}
NAMES = list(TREES)


def plant(name):
    """(A, perm, shapes, sign strings) of an input; a transposed input's patterns are written '+' first and exchanged here"""
    spine, leaves, more, transposed = TREES[name]
    nodes = tree(spine, leaves, more)
    if transposed:
        nodes = [(pat.translate(str.maketrans("+-", "-+")), p) for pat, p in nodes]
    return nodes, planted_tree_k2(nodes, PLANT_SEED, transposed)


def _planted(name):
    def make():
        _, (A, perm, _, _) = plant(name)
        return A, dict(relax=False, ordering="user", user_perm=perm)
    return make


INPUTS = {name: ("k2", "sparse", _planted(name)) for name in TREES}
# Regime "late" (theta over 16 decades, 5 % exact zeros, regularisations sqrt(eps)) only where the restatement factorises the input -- chosen on the
# CPU: TWO of the sixteen.  A planted front has about as many columns of A as rows (the K2 tests on random LPs: n = 2.7 m), so the '+' rows' Schur
# complement A D A' + Rd is as a rule numerically rank deficient once D spans 16 decades and is held up by Rd = sqrt(eps) alone: on the other fourteen the
# restatement meets a '+' pivot between -5e-06 and 0.0 (test_late_data_is_used_where_the_restatement_factorises_it).
LATE = ["tall_narrow", "mixed424"]
COMBOS = [(name, reg) for name in TREES for reg in ("ones", "mid", "late") if reg != "late" or name in LATE]
IDS = [f"{a}-{b}" for a, b in COMBOS]

_problems = {}


def problem(name, regime):
    """The mid problems are kept (the pair test uses them again); of the others the last one."""
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
    """name -> (planted shapes, analysed CPU handle, planted sign strings, nodes)"""
    out = {}
    for name in TREES:
        nodes, (A, perm, shapes, signs) = plant(name)
        kkt = tk.setup(A, tk.K2(), tk.Backend(device=-1, relax=False, ordering="user", user_perm=perm))
        out[name] = (shapes, kkt, signs, nodes, perm)
    return out


def signs_of(kkt):
    """The sign string of every analysed front, read back from perm"""
    g = kkt.symbolic
    s = np.where(g("perm") < kkt.n, "-", "+")
    return ["".join(s[c0: c0 + ns]) for c0, ns in zip(g("front_col0").tolist(), g("front_ns").tolist())]


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the inputs are what they claim to be
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_analysed_fronts_are_the_planted_ones(handles):
    for name, (shapes, kkt, signs, nodes, perm) in handles.items():
        g = kkt.symbolic
        assert np.array_equal(g("perm"), perm), name                       # the planted order is a postorder of its own tree: kept as given
        got = list(zip(g("front_ns").tolist(), g("front_f").tolist(), g("front_nchild").tolist(), signs_of(kkt)))
        assert got == [s + (p,) for s, p in zip(shapes, signs)], name     # front by front, in elimination order
        assert kkt.m + kkt.n <= 1100, name
        assert (signs[1][0] == "-") == TREES[name][3], name


def flip_set(pat):
    return {b for b in range(1, len(pat)) if pat[b - 1] != pat[b]}


def sweep_contents(trees):
    """The planted fronts of a table like TREES, helpers left out: (ns, rows below, planted children, pattern, is a root)"""
    fronts = []
    for name in trees:
        spine, leaves, more, transposed = trees[name]
        nodes = tree(spine, leaves, more)
        _, _, shapes, signs = planted_tree_k2(nodes, PLANT_SEED)          # (patterns as written: '+' first)
        for q, (pat, parent) in enumerate(nodes):
            ns, f, nch = shapes[2 * q + 1]
            assert signs[2 * q + 1] == pat and ns == len(pat)
            fronts.append((ns, f - ns, nch - 1, pat, parent < 0))
    return fronts


def check_sweep_contents(trees):
    fronts = sweep_contents(trees)
    check_shapes(fronts)
    check_signs(fronts)
    assert sum(1 for name in trees if trees[name][3]) >= 2                                  # transposed trees


def check_shapes(fronts):
    mixed = [(ns, rb, nch, pat, root) for ns, rb, nch, pat, root in fronts if "+" in pat and "-" in pat]
    assert len(mixed) == len(fronts)
    leaves = {(ns, rb) for ns, rb, nch, *_ in fronts if nch == 0}
    for ns in (2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257):          # pivot widths: over a few rows and over many
        assert any(a == ns and 0 < rb < 64 for a, rb in leaves), ("few rows", ns)
        assert any(a == ns and rb > 256 for a, rb in leaves), ("many rows", ns)
    for ns in (511, 512, 513, 768, 769):                                                    # signed split-K and its reduce; the signed chain
        assert any(a == ns and rb > 0 for a, rb in leaves), ns
    anyf = {(ns, rb) for ns, rb, *_ in fronts}
    for ns in (16, 17, 64, 257):                                                            # rows below
        for rb in (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257):
            assert (ns, rb) in anyf, ("rows below", ns, rb)
    for f in (63, 64, 65):
        assert (16, f - 16) in anyf and (17, f - 17) in anyf, ("f", f)
    interior = [(ns, nch) for ns, rb, nch, pat, root in fronts if nch > 0 and rb > 0]
    for ns in (17, 64, 65, 257):                                                            # extend-add targets with mixed signs
        assert any(a == ns and nch >= 2 for a, nch in interior), ("interior", ns)


def check_signs(fronts):
    pats = [pat for *_, pat, _ in fronts]
    for c in CUTS:                                                                          # a flip at every cut and one column past it
        assert any(c in flip_set(p) for p in pats), ("flip at", c - 1, c)
        assert any(c + 1 in flip_set(p) for p in pats), ("flip at", c, c + 1)
    for ns in (16, 17, 64, 257):
        assert alt(ns) in pats, ("alternating", ns)
    assert any(p == pm(len(p)) and len(p) > 16 for p in pats) and any(p == pm(len(p)) and len(p) > 64 for p in pats)
    assert any(p == lastm(len(p)) and len(p) > 2 for p in pats)
    p769 = [p for p in pats if len(p) == 769]
    assert p769 and all({256, 512} <= flip_set(p) and all(any(lo < b < lo + 256 for b in flip_set(p)) for lo in (0, 256, 512)) for p in p769)


def test_the_sweep_holds_every_shape_and_sign_pattern_it_is_for():
    check_sweep_contents(TREES)


def test_a_width_or_a_flip_moved_across_its_cut_is_noticed():
    """The assertion above has teeth: 64 -> 65 for one planted width, and the flips at 255 | 256 moved to 254 | 255."""
    moved = dict(TREES)
    sp_, lv, more, tr = TREES["rb127_129"]
    moved["rb127_129"] = (sp_, [(alt(65), k) if (pat, k) == (alt(64), 5) else (pat, k) for pat, k in lv], more, tr)
    with pytest.raises(AssertionError, match="rows below"):
        check_sweep_contents(moved)

    def shift(pat):
        return flips(len(pat), [255 if b == 256 else b for b in flip_set(pat)]) if len(pat) > 256 else pat
    moved = {name: ([shift(p) for p in sp_], [(shift(p), k) for p, k in lv], [([shift(p) for p in s], [(shift(p), k) for p, k in l]) for s, l in more], tr)
             for name, (sp_, lv, more, tr) in TREES.items()}
    with pytest.raises(AssertionError, match=r"'flip at', 255, 256"):         # (the signs alone: a flip moved inside a spine front also moves the rows below its children)
        check_signs(sweep_contents(moved))


def test_every_launch_kind_of_the_k1_sweep_is_reached(handles, k1_handles):
    k2 = {name: (v[0], v[1]) for name, v in handles.items()}
    assert missing_launch_kinds(k2) == missing_launch_kinds(k1_handles) == set()
    assert missing_launch_kinds(k2, without=["ns769"]) == {"CHAIN"}
    assert all(kkt.system == 1 for _, kkt in k2.values())
    red = {name: len(kkt.symbolic("reduce_tasks")) for name, (_, kkt) in k2.items()}
    assert all(red[name] > 0 for name in ("ns511_513", "ns512", "ns768", "ns769", "t_ns513")), red      # the signed split-K reduce


# per input: fronts in POTRF_SMALL, block columns in POTRF, in POTRF_WIDE, in TRSM_THIN, in TRSM, fronts in CHAIN, fronts in the small-front solve
# kernels, fronts in the sweeps -- the rule tables of tests/test_front_shapes.py applied to TREES (the helpers are one-column fronts: POTRF_SMALL,
# and the small solve up to 256 rows below).  A planted width moved across a cut changes a row.
CLASS_COUNTS = {
    "x257_rb1_17": (15, 5, 4, 19, 4, 0, 15, 5),   # N = 1096
    "x257_rb63_65": (12, 5, 4, 15, 5, 0, 11, 7),   # N = 1058
    "f63_65": (35, 11, 4, 43, 6, 0, 35, 15),   # N = 1071
    "x257_rb127_129": (10, 4, 5, 13, 5, 0, 7, 9),   # N = 1043
    "rb127_129": (25, 10, 1, 29, 4, 0, 25, 11),   # N = 578
    "x257_rb255_257": (13, 5, 4, 17, 4, 0, 5, 13),   # N = 1093
    "tall_narrow": (26, 11, 4, 31, 9, 0, 7, 33),   # N = 1070
    "tall_wide": (9, 1, 5, 9, 5, 0, 3, 11),   # N = 1039
    "ladder": (30, 10, 3, 33, 8, 0, 30, 12),   # N = 1090
    "ns511_513": (3, 2, 4, 4, 4, 0, 3, 3),   # N = 1060
    "ns512": (6, 2, 4, 5, 5, 0, 6, 4),   # N = 906
    "ns768": (2, 1, 3, 2, 3, 0, 1, 3),   # N = 803
    "ns769": (2, 0, 1, 2, 0, 1, 1, 3),   # N = 900: the two helpers small; the root 129 wide; the leaf, three block columns, in the chain
    "mixed424": (6, 3, 2, 8, 2, 0, 6, 4),   # N = 424: five helpers and the 16 small; 17, 64 and the last column of 257 in POTRF; 257's block column and the root wide
    "t_x257": (17, 5, 4, 19, 6, 0, 17, 7),   # N = 875
    "t_ns513": (6, 3, 3, 8, 3, 0, 6, 4),   # N = 680
}


def test_every_front_goes_to_the_kernels_its_shape_asks_for(handles):
    for name, (shapes, kkt, *_rest) in handles.items():
        potrf, trsm, solve, _ = classes_of(kkt)
        g = kkt.symbolic
        want_potrf, want_trsm, want_solve = {}, {}, {}
        for s, (ns, f) in enumerate(zip(g("front_ns").tolist(), g("front_f").tolist())):
            assert not g("front_single")[s]
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


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the three legs of tests/test_backward_error.py
# ---------------------------------------------------------------------------------------------------------------------------------
def test_restatement_is_inside_the_bound(pb):
    pb.assert_good_input()


def test_emulated_schedule_is_inside_the_bound(pb):
    emulator_leg(pb)


def test_mutation_one_small_entry_passes_the_normwise_criteria_and_fails_the_bound(pb):
    mutation_leg(pb)


def test_late_data_is_used_where_the_restatement_factorises_it():
    """One of the inputs left out of LATE: the restatement meets a pivot of the wrong sign there, so the regime is no test input (and would be a
    FAILURE of test_restatement_is_inside_the_bound, not a skip, were it listed)."""
    assert "ns769" not in LATE
    p = Problem("ns769", "late", INPUTS)
    assert "error" in p.stats and p.L is None


class WrongUpdateSign(Emulator):
    """The sign of ONE K column wrong in the update step only (k_update's staging): potrf and trsm keep the right one, so no pivot is reported"""

    def __init__(self, kkt, col):
        super().__init__(kkt)
        self.bad = col

    def _k3(self, T):
        self.sign[self.bad] *= -1.0
        try:
            super()._k3(T)
        finally:
            self.sign[self.bad] *= -1.0


def test_one_wrong_sign_in_the_update_step_leaves_the_bound():
    """Teeth for the signs: column 100 of a 257-column leaf (mid block; the pattern flips at the cuts only), its sign exchanged where the update
    multiplies by it.  Every pivot keeps its sign, nothing is reported (regime ones; with the mid data this column turns a later pivot and IS
    reported, columns 40 and 200 are not), and omega_hard of the factor leaves the bound: 1.1e-02 -> 2.7e+11."""
    pb = problem("x257_rb1_17", "ones")
    pb.assert_good_input()
    g = pb.kkt.symbolic
    s = [k for k, p in enumerate(signs_of(pb.kkt)) if p == at_cuts(257)][0]
    col = int(g("front_col0")[s]) + 100
    out = {}
    for who, em in (("emulator", Emulator(pb.kkt)), ("wrong sign", WrongUpdateSign(pb.kkt, col))):
        em.update(*pb.data[:3])
        assert em.fail_col is None
        out[who] = pb.check(who, dense_L_of_emulator(em, pb.system.N))["factor"]["hard"]
    assert out["emulator"] <= 1.0 < out["wrong sign"], out


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_factor_and_solves_are_inside_the_bound(pb, monkeypatch):
    """The device leg of tests/test_backward_error.py.  Regime mid is the leg with stale storage: TLPK_POISON=1 (the factor storage starts as NaNs),
    the ones data factorised first, then the mid data on the same handle."""
    if pb.regime != "mid":
        return device_leg(pb)
    monkeypatch.setenv("TLPK_POISON", "1")
    m, n = pb.A.shape
    device_leg(pb, who="device+stale", first=ipm_like_data(m, n, SEED, "ones")[:3])


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_pair_of_right_hand_sides(name):
    """tlpk_solve2_device with system = K2: both solutions bit for bit those of two single solves, and both inside the solve bound of the device's own factor."""
    pb = problem(name, "mid")
    pb.assert_good_input()
    _, kkt = make_handle(name, 0, INPUTS)
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
