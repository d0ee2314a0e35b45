"""Pivot verdict sweep: TLPK_NOT_POSDEF and tlpk_stats.fail_col at every kernel that takes the verdict and at every block cut inside it.

fail_col is the one signal of the factorisation that changes what the solvers do (the regularisation bumps, *fail_lp of the batch calls, the LPs a
streaming loop factorises again).  It is taken in k_single_factor, k_potrf_small, potrf_block / potrf_block_pair / potrf_block_wave / potrf_block_dpp
and in the potrf items of k_chain, each with index arithmetic of its own and each in a SIGNED variant; the other tests only ask for "raises".

Here a failure is PLANTED at a chosen permuted column (tests/pivot_reference.py: the recipes, decisive in exact arithmetic) of the inputs of the
front-shape sweeps (tests/test_front_shapes.py, tests/test_front_shapes_k2.py: a front on either side of every cut, and `classes_of`: which kernel
each block column goes to), and the reported column is compared with the first failing pivot of an unblocked L D L' in long double -- never with a
number that came from the code under test.  Columns: per analysed front the offsets {0, 1, ns - 1} and every o with o mod 16 in {0, 15} (regime ones),
{0, 15, 16, 63, 64, ns - 1} (regime mid); every isolated 1 x 1 front.

CPU: the reference verdict of every planted column is that column, with the margins of DESIGN.md section 1, "Pivot verdict sweep" on the pivots before it; the shortcut that
serves a whole sweep from one factorisation; the positions the sweep has to hold per kernel class; tests/emulate.py's model of the verdict on a sample
of each input (sign, exact zero, NaN, two plants, a walk in ascending order on ONE emulator); six wrong models, each caught.
GPU (-m gpu): per input the walk in ascending order on one handle -- PosDefException, fail_col, a refused solve -- and a good update whose factor is
bit for bit that of a fresh handle; two plants in one update; exact zeros and NaNs; the older diagonal-block kernels; graph replay against direct
enqueueing; *fail_lp and fail_col[k] of the batch calls on three stacked LPs.  The table of a run on an MI355X is profiles/pivot_verdict_sweep.txt."""
import time
from types import SimpleNamespace

import numpy as np
import pytest

import test_front_shapes as K1S
import test_front_shapes_k2 as K2S
import tulip_jl_amd as tk
from backward_error import System
from emulate import Emulator
from helpers import ipm_like_data
from pivot_reference import MARGIN, decisive, diag_sums, margins, pivots_ld, plant, planted_columns, planted_pivot, verdict
from test_backward_error import SEED, _dense
from test_front_shapes import classes_of
from test_set_values import factor_entries

DENSE_SHAPES = [(129, 17), (257, 33), (333, 1001)]           # the last goes through the split-K SYRK and its reduce
SINGLES = "singles"


def _singles():
    """[A0 I] with a third of the rows empty but for their slack (tests/test_symbolic.py), at 900 rows: more than 256 isolated 1 x 1 fronts, so that
    singles 255 | 256 lie on either side of a workgroup of k_single_factor"""
    from test_symbolic import singleton_rows_matrix
    return singleton_rows_matrix(m=900, n0=600), {}


def _t_ns769():
    """ns769 of the K2 sweep TRANSPOSED (every sign exchanged): the chain's last column, the one-column partial block at offset 768, is a '-' node in
    the sixteen inputs of the K2 sweep; here it is a '+' node"""
    from lp_generators import planted_tree_k2
    spine, leaves, more, _ = K2S.TREES["ns769"]
    nodes = [(pat.translate(str.maketrans("+-", "-+")), p) for pat, p in K2S.tree(spine, leaves, more)]
    A, perm, _, _ = planted_tree_k2(nodes, K2S.PLANT_SEED, True)
    return A, dict(relax=False, ordering="user", user_perm=perm)


# (family, name) -> (kind of the factored system, backend class, matrix + backend keywords): the tables of the two front-shape sweeps, as they are
INPUTS = {("k1", name): K1S.INPUTS[name] for name in K1S.TREES}
INPUTS.update({("k2", name): K2S.INPUTS[name] for name in K2S.TREES})
INPUTS.update({("dense", f"{m}x{n}"): ("k1", "dense", _dense(m, n)) for m, n in DENSE_SHAPES})
INPUTS[("k1", SINGLES)] = ("k1", "sparse", _singles)
INPUTS[("k2", "t_ns769")] = ("k2", "sparse", _t_ns769)
K1_NAMES, K2_NAMES, DENSE_NAMES = list(K1S.TREES), list(K2S.TREES) + ["t_ns769"], [f"{m}x{n}" for m, n in DENSE_SHAPES]
assert len(K1_NAMES) == 13 and len(K2_NAMES) == 16 + 1
CLASSES = ("single", "POTRF_SMALL", "POTRF", "POTRF_WIDE", "CHAIN")
ALL_POS = {"first", "last_full", "next_first", "last_partial", "cut16_left", "cut16_right"}
# the positions a kernel class can hold at all: an isolated front is one column; a one-wave front has at most 16 columns (no cut inside it); a block
# column of POTRF is at most one 64-block
REQUIRED = {"single": {"first"}, "POTRF_SMALL": {"first", "last_partial"}, "POTRF": ALL_POS - {"next_first"}, "POTRF_WIDE": ALL_POS, "CHAIN": ALL_POS}


def positions(o, ns):
    """What column o of a front of ns pivot columns is to the block that holds it: block columns of 256, in them blocks of 64, in them panels of 16"""
    k0 = 256 * (o // 256)
    w = min(256, ns - k0)
    b, j = divmod(o - k0, 64)
    bw = min(64, w - 64 * b)
    tags = set()
    if j == 0:
        tags.add("first")
    if j == 0 and b > 0:
        tags.add("next_first")                 # the first column of the block after a full one
    if j == bw - 1:
        tags.add("last_full" if bw == 64 else "last_partial")
    if j % 16 == 15 and j + 1 < bw:
        tags.add("cut16_left")
    if j % 16 == 0 and j > 0:
        tags.add("cut16_right")
    return tags


class Case:
    """One input: the analysed (CPU) handle, the kernel class and the positions of every column, and per regime the reference (`ref`)"""

    def __init__(self, fam, name):
        self.fam, self.name = fam, name
        self.kind, self.backend, make = INPUTS[(fam, name)]
        self.A, self.kw = make()
        self.kkt = self.handle(-1)
        g = self.kkt.symbolic
        self.perm = g("perm")
        self.N = len(self.perm)
        self.col0, self.ns, self.single = g("front_col0").tolist(), g("front_ns").tolist(), g("front_single").tolist()
        potrf = classes_of(self.kkt)[0]
        self.cls, self.tags, self.front = [None] * self.N, [None] * self.N, [None] * self.N
        for s, (c0, ns) in enumerate(zip(self.col0, self.ns)):
            for o in range(ns):
                self.cls[c0 + o] = "single" if self.single[s] else potrf[(s, 256 * (o // 256))]
                self.tags[c0 + o] = positions(o, ns)
                self.front[c0 + o] = s
        assert None not in self.cls
        self._ref = {}

    def handle(self, device):
        if self.backend == "dense":
            return tk.setup(self.A, tk.K1(), tk.DenseBackend(device=device))
        return tk.setup(self.A, tk.K2() if self.kind == "k2" else tk.K1(), tk.Backend(device=device, **self.kw))

    def sign(self, c):
        return -1.0 if (self.kind == "k2" and self.perm[c] < self.A.shape[1]) else 1.0

    def data(self, regime):
        m, n = self.A.shape
        return ipm_like_data(m, n, SEED, regime)

    def system(self, data):
        return System(self.kind, self.A, self.perm, data)

    def ref(self, regime):
        """ONE long-double factorisation of the unplanted data; of the system only what a plant needs is kept (K^, F, P are 45 MB an input)"""
        if regime not in self._ref:
            sysm = self.system(self.data(regime))
            d = pivots_ld(sysm)
            assert verdict(sysm.sign, d) is None, (self.name, regime, "the unplanted data does not factorise")
            mg, before = margins(sysm, d)
            light = SimpleNamespace(kind=sysm.kind, perm=sysm.perm, n=sysm.n, N=sysm.N, data=sysm.data)
            self._ref[regime] = SimpleNamespace(system=light, sign=sysm.sign.copy(), d=d, margin=mg, before=before, data=sysm.data)
        return self._ref[regime]

    def planted(self, regime, c, what="sign"):
        r = self.ref(regime)
        if getattr(r, "sums", None) is None:
            r.sums = diag_sums(self.kind, self.A, r.data)
        return plant(self.kind, self.A, r.data, int(self.perm[c]), what, sums=r.sums)

    def reference_verdict(self, regime, c, what="sign"):
        """(verdict, planted pivot) of the data planted at column c, from the pivots of the unplanted data"""
        r = self.ref(regime)
        d = r.d.copy()
        d[c] = planted_pivot(r.system, r.d, c, self.planted(regime, c, what))
        return verdict(r.sign[: c + 1], d[: c + 1]), d[c]

    def columns(self, regime):
        """The planted columns of the regime that meet the margin on every pivot before them, and those left out"""
        r = self.ref(regime)
        cols = planted_columns(self.kkt, regime)
        keep = [c for c in cols if r.before[c] >= MARGIN]
        return keep, [c for c in cols if r.before[c] < MARGIN]

    def full_reference(self, regime, c, what):
        """A factorisation of its own for a plant that moves more than one entry (exact zero): (verdict, pivots, margins before)"""
        sysm = self.system(self.planted(regime, c, what) + self.ref(regime).data[3:])
        d = pivots_ld(sysm)
        return verdict(sysm.sign, d), d, margins(sysm, d)[1]


_cases = {}


def case(fam, name):
    if (fam, name) not in _cases:
        _cases[(fam, name)] = Case(fam, name)
    return _cases[(fam, name)]


ALL = [("k1", n) for n in K1_NAMES] + [("k2", n) for n in K2_NAMES] + [("dense", n) for n in DENSE_NAMES] + [("k1", SINGLES)]
ALL_IDS = [f"{f}-{n}" for f, n in ALL]


def single_columns(cs):
    """The isolated fronts in the order k_single_factor takes them (front order): singles 0, 255, 256 and the last"""
    cols = [c0 for c0, one in zip(cs.col0, cs.single) if one]
    return cols, sorted({cols[0], cols[255], cols[256], cols[-1]})


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the reference
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,name", ALL, ids=ALL_IDS)
def test_the_reference_verdict_of_every_planted_column_is_that_column(fam, name):
    """Sections 1 and 2 of the recipe on the CPU, before anything runs on a GPU: the planted pivot decides by itself (wrong sign by 0.5 at least) and
    every pivot before it keeps its sign by 1e4 N u F_cc.  ones: no column may be left out; mid: at most 5 %, printed."""
    cs = case(fam, name)
    for regime in ("ones", "mid"):
        r = cs.ref(regime)
        keep, out = cs.columns(regime)
        if regime == "ones":
            assert not out, (name, "ones", out)
        assert len(out) <= 0.05 * (len(keep) + len(out)), (name, regime, out)
        worst = np.inf
        for c in keep:
            v, dc = cs.reference_verdict(regime, c)
            assert decisive(cs.sign(c), dc) and abs(dc) >= 0.5, (name, regime, c, dc)
            assert v == c, (name, regime, c, v)
            worst = min(worst, r.before[c])
        print(f"PV-REF {fam}-{name:15s} {regime:4s} N={cs.N:5d} planted={len(keep):4d} left out={out} smallest margin before a planted column = {worst:.3e} N u F_cc")
    if name == SINGLES:
        cols, picked = single_columns(cs)
        assert len(cols) > 257 and set(picked) <= set(cs.columns("ones")[0])


SHORTCUT = [("k1", "interior", "mid"), ("k2", "tall_narrow", "mid"), ("k2", "t_ns513", "ones"), ("dense", "129x17", "mid")]


@pytest.mark.parametrize("fam,name,regime", SHORTCUT, ids=[f"{f}-{n}-{r}" for f, n, r in SHORTCUT])
def test_one_factorisation_serves_the_sweep(fam, name, regime):
    """The shortcut against a long-double factorisation of the planted data itself, at the first, a middle and the last planted column (K2: one node of
    each sign among them): the pivots before the column bit for bit, the planted pivot to the last bits of long double, the same verdict."""
    cs = case(fam, name)
    r = cs.ref(regime)
    keep = cs.columns(regime)[0]
    pick = {keep[0], keep[len(keep) // 2], keep[-1]}
    if cs.kind == "k2":
        pick |= {[c for c in keep if cs.sign(c) == s][len(keep) // 4] for s in (-1.0, 1.0)}
    for c in sorted(pick):
        v, dc = cs.reference_verdict(regime, c)
        vf, d, _ = cs.full_reference(regime, c, "sign")
        assert vf == v == c
        assert d[:c].tobytes() == r.d[:c].tobytes()
        assert abs(d[c] - dc) <= 2.0 ** -58 * (abs(dc) + abs(r.d[c])), (c, d[c], dc)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: what the sweep holds
# ---------------------------------------------------------------------------------------------------------------------------------
def contents(fam, names, regime="ones"):
    """{(kernel class, position, sign of the node)} over the planted columns of the inputs"""
    out = set()
    for name in names:
        cs = case(fam, name)
        for c in planted_columns(cs.kkt, regime):
            out |= {(cs.cls[c], t, cs.sign(c)) for t in cs.tags[c]}
    return out


def missing_positions(fam, names, signs):
    have = contents(fam, names)
    classes = CLASSES if fam == "k1" else CLASSES[1:]              # (an augmented system has no isolated node)
    return {(k, t, s) for k in classes for t in REQUIRED[k] for s in signs} - have


def test_the_sweep_holds_every_position_in_every_kernel_class():
    """Per potrf class (classes_of: the isolated fronts, POTRF_SMALL, POTRF, POTRF_WIDE, CHAIN): the first column of a block; the last column of a full
    64-block and the first of the next; the last column of a partial block; both sides of a 16-column cut -- for K1, and for K2 at a node of each sign."""
    assert missing_positions("k1", K1_NAMES + [SINGLES], (1.0,)) == set()
    assert missing_positions("k2", K2_NAMES, (1.0, -1.0)) == set()
    # teeth: ns769 is the only carrier of the chain
    gone = missing_positions("k1", [n for n in K1_NAMES if n != "ns769"] + [SINGLES], (1.0,))
    assert gone == {("CHAIN", t, 1.0) for t in ALL_POS}
    gone = missing_positions("k2", [n for n in K2_NAMES if "ns769" not in n], (1.0, -1.0))
    assert gone == {("CHAIN", t, s) for t in ALL_POS for s in (1.0, -1.0)}
    assert missing_positions("k2", [n for n in K2_NAMES if n != "t_ns769"], (1.0, -1.0)) == {("CHAIN", "last_partial", 1.0)}
    # the mid offsets reach a second block column (ns - 1 of a 257-column front): the plant that notices a column reported without k0
    assert any(c - cs.col0[cs.front[c]] >= 256 for cs in [case("k1", "x257_rb1_17")] for c in planted_columns(cs.kkt, "mid"))


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the emulator's model of the verdict
# ---------------------------------------------------------------------------------------------------------------------------------
def emulator_of(cs):
    if cs.backend == "dense":
        from test_dense_backend import DenseEmulator
        return DenseEmulator
    return Emulator


def sample(cs, regime="mid"):
    """The emulator's share of the sweep (an update of tests/emulate.py costs up to a second): per (kernel class, position, sign) the first column of the
    regime's set that holds it, and the first and the last column that lie in a second block column"""
    keep = cs.columns(regime)[0]
    first = {}
    for c in keep:
        for t in cs.tags[c]:
            first.setdefault((cs.cls[c], t, cs.sign(c)), c)
    later = [c for c in keep if c - cs.col0[cs.front[c]] >= 256]
    return sorted(set(first.values()) | set(later[:1] + later[-1:]))


def special_columns(cs, regime="ones"):
    """One planted column per kernel class of the input for the exact-zero and the NaN plants: the last of the class that is the last column of a partial
    block, else the last of the class"""
    keep = cs.columns(regime)[0]
    out = {}
    for c in keep:
        if cs.cls[c] not in out or "last_partial" in cs.tags[c] or "last_partial" not in cs.tags[out[cs.cls[c]]]:
            out[cs.cls[c]] = c
    return out


def nan_columns(cs, regime="ones"):
    """Where the NaN goes.  K1: the column of the input's highest kernel class.  K2: per sign of the node the last planted column of a front of more than one column"""
    if cs.kind == "k1":
        spec = special_columns(cs, regime)
        return [spec[max(spec, key=CLASSES.index)]]
    keep = [c for c in cs.columns(regime)[0] if cs.ns[cs.front[c]] > 1]
    return sorted([c for c in keep if cs.sign(c) == s][-1] for s in (1.0, -1.0))


def pair_columns(cs, regime="ones"):
    """Pairs c1 < c2 planted in ONE update: fronts of different kernel classes with neither an ancestor of the other; a front and an ancestor of it; two
    64-blocks of one POTRF_WIDE block column.  Per kind the first pair found."""
    keep = cs.columns(regime)[0]
    parent = cs.kkt.symbolic("front_parent").tolist()

    def ancestors(s):
        out = set()
        while parent[s] >= 0:
            s = parent[s]
            out.add(s)
        return out
    anc = {s: ancestors(s) for s in set(cs.front[c] for c in keep)}
    pairs = {}
    for a in keep:
        for b in keep:
            if b <= a:
                continue
            fa, fb = cs.front[a], cs.front[b]
            if fa != fb and cs.cls[a] != cs.cls[b] and fb not in anc[fa] and fa not in anc[fb]:
                pairs.setdefault("apart", (a, b))
            if fb in anc[fa]:
                pairs.setdefault("ancestor", (a, b))
            oa, ob = a - cs.col0[fa], b - cs.col0[fb]
            if fa == fb and cs.cls[a] == "POTRF_WIDE" and oa // 256 == ob // 256 and oa // 64 != ob // 64:
                pairs.setdefault("one block column", (a, b))
        if len(pairs) == 3:
            break
    return pairs


def plant_two(cs, regime, a, b):
    """The data planted at a and at b: the two recipes move different entries of (theta, regP, regD)"""
    base = cs.ref(regime).data[:3]
    pa, pb_ = cs.planted(regime, a), cs.planted(regime, b)
    return tuple(np.where(np.asarray(x) != np.asarray(z), x, y) for x, y, z in zip(pa, pb_, base))


def emulator_leg(cs, make=None, columns=None, parts=("walk", "zero", "nan", "pair")):
    """tests/emulate.py against the reference on ONE emulator object: the sample in ASCENDING order (a verdict that is not cleared would win the min), then
    an exact zero and a NaN (K2: NaNs), two plants in one update, and a good update that reports nothing."""
    em = (make or emulator_of(cs))(cs.kkt)
    em.planted_failures = True                 # (behind a replaced pivot the columns may overflow: no floating-point warnings from these updates)
    if "walk" in parts:
        for c in (sample(cs) if columns is None else columns):
            v, _ = cs.reference_verdict("mid", c)
            em.update(*cs.planted("mid", c))
            assert em.fail_col == v == c, (cs.name, "mid", c, em.fail_col)
    spec = special_columns(cs)
    if "zero" in parts and cs.kind == "k1":
        c = spec[max(spec, key=CLASSES.index)]
        v, d, before = cs.full_reference("ones", c, "zero")
        assert v == c and d[c] == 0.0 and before[c] >= MARGIN, (cs.name, c, v, d[c])
        em.update(*cs.planted("ones", c, "zero"))
        assert em.fail_col == c, (cs.name, "zero", c, em.fail_col)
    if "nan" in parts:
        for c in nan_columns(cs):
            v, dc = cs.reference_verdict("ones", c, "nan")
            assert v == c and np.isnan(dc)
            em.update(*cs.planted("ones", c, "nan"))
            assert em.fail_col == c, (cs.name, "nan", c, em.fail_col)
    if "pair" in parts:
        pairs = pair_columns(cs)
        assert pairs and ("ancestor" in pairs or len(cs.ns) == 1), cs.name
        for kind_ in sorted(pairs):                                          # every kind the input has (a front and an ancestor of it: every input of more than one front)
            a, b = pairs[kind_]
            em.update(*plant_two(cs, "ones", a, b))
            assert em.fail_col == a, (cs.name, kind_, a, b, em.fail_col)
    em.update(*cs.ref("mid").data[:3])
    assert em.fail_col is None


EMULATED = [("k1", n) for n in ("interior", "small_only", "ns769", SINGLES)] + [("k2", n) for n in ("mixed424", "ns769")] \
    + [("dense", "129x17")]


@pytest.mark.parametrize("fam,name", EMULATED, ids=[f"{f}-{n}" for f, n in EMULATED])
def test_the_emulators_verdict_is_the_reference_verdict(fam, name):
    emulator_leg(case(fam, name))


# Six wrong models of the verdict, each in a subclass of the emulator; each must make the emulator leg fail on the input named beside it.
class ZeroPasses(Emulator):                     # d < 0 in place of not (d > 0): an exact zero or a NaN passes
    def _pivot_fails(self, sj, d):
        return sj * d < 0


class WithoutCol0(Emulator):                    # the column inside the front
    def _report(self, col0, k0, j):
        super()._report(0, k0, j)


class WithoutK0(Emulator):                      # the column inside the block column
    def _report(self, col0, k0, j):
        super()._report(col0, 0, j)


class LargestWins(Emulator):                    # max in place of min
    def _report(self, col0, k0, j):
        col = col0 + k0 + j
        self.fail_col = col if self.fail_col is None else max(self.fail_col, col)


class NeverCleared(Emulator):                   # the status word survives an update
    def _clear_verdict(self):
        self.fail_col = getattr(self, "fail_col", None)


class SignIgnored(Emulator):                    # K2 judged as K1
    def _sign_of(self, col):
        return 1.0


MUTATIONS = [(ZeroPasses, "k1", "small_only", ("zero", "nan")), (WithoutCol0, "k1", "small_only", ("walk",)), (WithoutK0, "k1", "x257_rb1_17", ("walk",)),
             (LargestWins, "k1", "small_only", ("pair",)), (NeverCleared, "k1", "small_only", ("walk",)), (SignIgnored, "k2", "mixed424", ("walk",))]


@pytest.mark.parametrize("mutant,fam,name,parts", MUTATIONS, ids=[m[0].__name__ for m in MUTATIONS])
def test_a_wrong_model_of_the_verdict_is_caught(mutant, fam, name, parts):
    cs = case(fam, name)
    columns = None
    if mutant is WithoutK0:                     # (the columns of the second block columns, and one before them)
        columns = [c for c in sample(cs) if c - cs.col0[cs.front[c]] >= 256]
        assert columns
    emulator_leg(cs, parts=parts, columns=columns)                       # the leg passes with the model as it is ...
    with pytest.raises(AssertionError):
        emulator_leg(cs, make=mutant, parts=parts, columns=columns)      # ... and fails with the wrong one


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def device_update(kkt, data):
    """One update of planted data: the column the device names, None if it raised nothing"""
    try:
        tk.update(kkt, *data)
    except tk.PosDefException:
        col = kkt.stats()["fail_col"]
        assert col >= 0
        return col
    return None


def refused(kkt, cs):
    m, n = cs.A.shape
    with pytest.raises(RuntimeError):
        tk.solve(np.zeros(n), np.zeros(m), kkt, np.ones(m), np.ones(n))          # not factored


def walk(cs, kkt, regimes=("ones", "mid"), wrong=None):
    """The planted columns of each regime in ASCENDING order on one handle (a stale smaller verdict of the update before would win the min): the device's
    column against the reference's.  Returns the columns planted per kernel class; the mismatches go to `wrong`."""
    count = {}
    wrong = [] if wrong is None else wrong
    for regime in regimes:
        for c in cs.columns(regime)[0]:
            v, _ = cs.reference_verdict(regime, c)
            assert v == c
            got = device_update(kkt, cs.planted(regime, c))
            if got != c:
                wrong.append((regime, c, cs.cls[c], got))
            refused(kkt, cs)
            count[cs.cls[c]] = count.get(cs.cls[c], 0) + 1
    return count, wrong


def good_update_equals_a_fresh_handle(cs, kkt):
    """After the failures: one good update, whose factor is bit for bit that of the same data on a handle that never failed, and so is a solve through it.
    The factor: every entry of L (test_set_values.factor_entries).  factor_panels() has more words than these -- rows f .. lda - 1 of a column, the
    never-stored blocks above the diagonal blocks, the words between two panels -- which no update writes and no solve reads: a handle finds there what
    the allocation held before (on an MI355X: words of handles this process had closed, different from run to run)."""
    th, rp, rd, xp, xd = cs.ref("mid").data
    m, n = cs.A.shape
    out = []
    fresh = cs.handle(0)
    for h in (kkt, fresh):
        tk.update(h, th, rp, rd)
        assert h.stats()["fail_col"] < 0
        dx, dy = np.zeros(n), np.zeros(m)
        tk.solve(dx, dy, h, xp, xd)
        out.append((factor_entries(h, h.factor_panels()).tobytes(), dx.tobytes(), dy.tobytes()))
    fresh.close()
    assert out[0][0] == out[1][0], (cs.name, "the factor after the failed updates differs from a fresh handle's")
    assert out[0][1:] == out[1][1:], (cs.name, "the solution after the failed updates differs from a fresh handle's")


def sweep_of(fam, name):
    cs = case(fam, name)
    t0 = time.time()
    cs.ref("ones"), cs.ref("mid")
    t1 = time.time()
    kkt = cs.handle(0)
    for what in ("perm", "front_col0", "front_ns"):
        assert np.array_equal(kkt.symbolic(what), cs.kkt.symbolic(what)), what
    count, wrong = walk(cs, kkt)
    good_update_equals_a_fresh_handle(cs, kkt)
    kkt.close()
    per = " ".join(f"{k}={count.get(k, 0)}" for k in CLASSES)
    print(f"PV {fam}-{name:15s} N={cs.N:5d} planted: {per} | mismatches={len(wrong)} | reference {t1 - t0:.1f} s, device {time.time() - t1:.1f} s")
    assert not wrong, (name, wrong[:10])


@pytest.mark.gpu
@pytest.mark.parametrize("name", K1_NAMES)
def test_device_verdicts_k1(name):
    sweep_of("k1", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", K2_NAMES)
def test_device_verdicts_k2(name):
    sweep_of("k2", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", DENSE_NAMES)
def test_device_verdicts_dense(name):
    sweep_of("dense", name)


@pytest.mark.gpu
def test_device_verdicts_of_the_isolated_fronts():
    """k_single_factor: singles 0, 255 | 256 (either side of a workgroup) and the last one first, then the whole sweep of the input"""
    cs = case("k1", SINGLES)
    cols, picked = single_columns(cs)
    kkt = cs.handle(0)
    for c in picked:
        assert cs.cls[c] == "single" and cs.reference_verdict("ones", c)[0] == c
        assert device_update(kkt, cs.planted("ones", c)) == c, c
        refused(kkt, cs)
    kkt.close()
    sweep_of("k1", SINGLES)


PAIRED = [("k1", n) for n in ("interior", "ladder", "rb63_65", "ns769")] + [("k2", n) for n in ("tall_narrow", "mixed424")]


@pytest.mark.gpu
@pytest.mark.parametrize("fam,name", PAIRED, ids=[f"{f}-{n}" for f, n in PAIRED])
def test_device_two_plants_in_one_update(fam, name):
    """c1 < c2 in one update: the smaller column is named -- across kernels that run side by side, between a front and its ancestor, between two 64-blocks
    of one block column"""
    cs = case(fam, name)
    pairs = pair_columns(cs)
    assert "ancestor" in pairs and (name == "ns769" or "apart" in pairs)
    kkt = cs.handle(0)
    for kind_, (a, b) in pairs.items():
        assert cs.reference_verdict("ones", a)[0] == a and cs.reference_verdict("ones", b)[0] == b
        got = device_update(kkt, plant_two(cs, "ones", a, b))
        print(f"PV2 {fam}-{name:12s} {kind_:16s} columns {a} ({cs.cls[a]}) < {b} ({cs.cls[b]}): device {got}")
        assert got == a, (kind_, a, b, got)
    kkt.close()


def test_the_pairs_hold_every_kind():
    kinds = set()
    for fam, name in PAIRED:
        kinds |= set(pair_columns(case(fam, name)))
    assert kinds == {"apart", "ancestor", "one block column"}


SPECIAL = ["interior", "ladder", "ns513", "ns769"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", SPECIAL)
def test_device_exact_zero_and_nan_pivots(name):
    """One column per kernel class of the input: an exactly zero pivot (theta = inf on every column of the row, regD = 0) and a NaN pivot are reported at
    their column (the comment above potrf_block promises both)"""
    cs = case("k1", name)
    kkt = cs.handle(0)
    for cls, c in sorted(special_columns(cs).items(), key=lambda kv: kv[1]):
        v, d, before = cs.full_reference("ones", c, "zero")
        assert v == c and d[c] == 0.0 and before[c] >= MARGIN
        got = device_update(kkt, cs.planted("ones", c, "zero"))
        assert got == c, (name, cls, "zero", c, got)
        v, dc = cs.reference_verdict("ones", c, "nan")
        assert v == c and np.isnan(dc)
        got = device_update(kkt, cs.planted("ones", c, "nan"))
        assert got == c, (name, cls, "nan", c, got)
    good_update_equals_a_fresh_handle(cs, kkt)
    kkt.close()


def test_the_special_plants_reach_every_kernel_class():
    assert set().union(*(set(special_columns(case("k1", name))) for name in SPECIAL)) == set(CLASSES)


@pytest.mark.gpu
def test_device_nan_pivots_k2():
    cs = case("k2", "tall_narrow")
    cols = nan_columns(cs)
    assert {cs.sign(c) for c in cols} == {1.0, -1.0}
    kkt = cs.handle(0)
    for c in cols:
        v, dc = cs.reference_verdict("ones", c, "nan")
        assert v == c and np.isnan(dc)
        assert device_update(kkt, cs.planted("ones", c, "nan")) == c, c
    kkt.close()


VARIANTS = [("k1", "rb63_65"), ("k2", "x257_rb63_65")]


@pytest.mark.gpu
@pytest.mark.parametrize("fam,name", VARIANTS, ids=[f"{f}-{n}" for f, n in VARIANTS])
def test_device_verdicts_of_the_other_diagonal_block_kernels(fam, name, monkeypatch):
    """TLPK_POTRF_MODE 3 (potrf_block_dpp, the default), 2 (potrf_block_pair), 1 (potrf_block_wave), 0 (potrf_block), re-read at every launch under
    TLPK_POTRF_DYN: the ones sweep of an input with POTRF and POTRF_WIDE block columns"""
    monkeypatch.setenv("TLPK_POTRF_DYN", "1")
    cs = case(fam, name)
    assert {"POTRF", "POTRF_WIDE"} <= set(cs.cls)
    kkt = cs.handle(0)
    for mode in ("3", "2", "1", "0"):
        monkeypatch.setenv("TLPK_POTRF_MODE", mode)
        count, wrong = walk(cs, kkt, regimes=("ones",))
        print(f"PV-MODE {fam}-{name} mode {mode}: planted {sum(count.values())} mismatches {len(wrong)}")
        assert not wrong, (mode, wrong[:10])
        tk.update(kkt, *cs.ref("ones").data[:3])
    kkt.close()


@pytest.mark.gpu
def test_device_verdicts_under_graph_replay_and_direct_enqueue(monkeypatch):
    """TLPK_GRAPH=1 (hipGraph replay of the static schedule) and 0 (direct enqueueing): the same columns"""
    cs = case("k1", "interior")
    for mode in ("1", "0"):
        monkeypatch.setenv("TLPK_GRAPH", mode)
        kkt = cs.handle(0)
        count, wrong = walk(cs, kkt, regimes=("ones",))
        assert not wrong, (mode, wrong[:10])
        good_update_equals_a_fresh_handle(cs, kkt)
        kkt.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# Batch ownership: *fail_lp of tlpk_ipm_batch_factor and fail_col[k] of tlpk_ipm_batch_factor_each (the host's mapping of a column to its LP, k_fold_fail)
# ---------------------------------------------------------------------------------------------------------------------------------
# The batch calls take ONE regP and ONE regD per LP, so a plant is a value of regD[k].  S_k = M_k + r I with M_k = A_k D_k A_k' in the block's permuted order:
#   first column of the block   r = -max_i (M_k)_ii - 1: every diagonal entry of S_k is <= -1, the block's first pivot is its diagonal entry.
#   last column of the block    -r halfway between lambda_min(M_k) and lambda_min of its leading submatrix without the last column (interlacing: the second is
#                               not smaller): every leading block but the whole one is positive definite, S_k has one negative eigenvalue, so every pivot of
#                               the block is positive but the last.
# The reference decides as everywhere in this file; its margin is MARGIN N u F_cc on every pivot of an LP up to and INCLUDING its failing one (these plants do
# not reach |d| >= 0.5: the gap of two eigenvalues of a 2 .. 5 row block is what it is; 1e4 N u F_cc is what no kernel's rounding turns).
def lp_columns(perm, ro):
    """Per LP the permuted columns of its rows, ascending"""
    return [np.nonzero((perm >= ro[k]) & (perm < ro[k + 1]))[0] for k in range(len(ro) - 1)]


def batch_plant(A, perm, ro, th, gP_k, k, where):
    """regD[k] that plants a failure at the first / the last permuted column of LP k's block (K1), regP[k] = gP_k"""
    cols = lp_columns(perm, ro)[k]
    Ak = A.toarray()[perm[cols]]
    M = (Ak / (th + gP_k)) @ Ak.T                    # (the columns of the other LPs are zero in these rows)
    if where == "first":
        return -float(np.diag(M).max()) - 1.0
    lam, lam_lead = np.linalg.eigvalsh(M)[0], np.linalg.eigvalsh(M[:-1, :-1])[0]
    assert lam_lead > lam > 0
    return -0.5 * (lam + lam_lead)


def batch_reference(A, perm, ro, co, th, rP, rD):
    """(fail_col per LP, the LP that owns the smallest) of a stacked K1 system with per-LP regularisations, from the long-double pivots: the LPs' blocks do not
    meet, so the pivots of one LP do not depend on what was done to another's failing pivot."""
    m, n = A.shape
    data = (th, np.repeat(rP, np.diff(co)), np.repeat(rD, np.diff(ro)), np.zeros(m), np.zeros(n))
    sysm = System("k1", A, perm, data)
    d = pivots_ld(sysm)
    mg = margins(sysm, d)[0]
    fail_col = np.full(len(ro) - 1, -1, dtype=np.int64)
    for k, cols in enumerate(lp_columns(perm, ro)):
        for c in cols:
            assert abs(mg[c]) >= MARGIN, (k, c, mg[c])
            if not d[c] > 0:
                fail_col[k] = c
                break
    bad = fail_col[fail_col >= 0]
    return fail_col, (int(np.argmax(fail_col == bad.min())) if bad.size else -1)


BATCH_PLANS = [[(k, w)] for k in range(3) for w in ("first", "last")] + [[(0, "last"), (1, "first"), (2, "last")], [(0, "first"), (1, "last"), (2, "first")],
                                                                         [(1, "last"), (2, "last")]]


def batch_inputs(device):
    from test_hsd_batch import stacked_handle
    A, ro, co, vecs = stacked_handle()                # the three stacked LPs (3 x 7, 5 x 9, 2 x 4) of tests/test_hsd_batch.py and tests/test_batch_retry.py
    kkt = tk.setup(A, tk.K1(), tk.Backend(device=device, row_block=np.repeat(np.arange(3), np.diff(ro))))
    return A, ro, co, vecs, kkt


def test_the_batch_plants_name_the_first_and_the_last_column_of_each_block():
    """The recipes on the CPU with theta_inv = 1 standing in for the iterate's (the GPU leg reads the iterate's and asserts the same before it runs a plant)"""
    A, ro, co, vecs, kkt = batch_inputs(-1)
    perm = kkt.symbolic("perm")
    th, gP, gD = np.ones(A.shape[1]), np.full(3, 1e-4), np.full(3, 1e-4)
    cols = lp_columns(perm, ro)
    assert sorted(np.concatenate(cols).tolist()) == list(range(A.shape[0])) and all(len(c) >= 2 for c in cols)
    assert batch_reference(A, perm, ro, co, th, gP, gD)[1] == -1
    for plan in BATCH_PLANS:
        rD = gD.copy()
        for k, where in plan:
            rD[k] = batch_plant(A, perm, ro, th, gP[k], k, where)
        fc, lp = batch_reference(A, perm, ro, co, th, gP, rD)
        want = {k: int(cols[k][0] if where == "first" else cols[k][-1]) for k, where in plan}
        assert fc.tolist() == [want.get(k, -1) for k in range(3)], (plan, fc)
        assert lp == min(want, key=want.get)
    kkt.close()


@pytest.mark.gpu
def test_device_batch_verdicts_name_the_reference_column_and_its_lp():
    """One stacked batch of three LPs; plants at the first and the last column of each LP's block, one LP at a time in ascending order of the column and
    several LPs in one update: *fail_lp and fail_col[k] against the long-double reference.  Nothing here is read from stats(); theta_inv is the iterate's,
    read back with tlpk_ipm_get (an INPUT of the factorisation, formed by another kernel)."""
    import ctypes as C
    from test_batch_retry import each
    from test_hsd_batch import load_batch
    from tulip_jl_amd import _lib
    L = _lib.lib()
    pu8, pd = _lib.as_pu8, _lib.as_pd
    A, ro, co, vecs, kkt = batch_inputs(0)
    m, n = A.shape
    rc, msg = load_batch(kkt, 3, ro, co, vecs)
    assert rc == _lib.OK, msg
    perm = kkt.symbolic("perm")
    cols = lp_columns(perm, ro)
    ones, gP, gD = np.ones(3, dtype=np.uint8), np.full(3, 1e-4), np.full(3, 1e-4)
    fail = C.c_int64(-7)
    assert L.tlpk_ipm_batch_factor(kkt._h, pu8(ones), pd(gP), pd(gD), C.byref(fail)) == _lib.OK and fail.value == -1
    th = np.empty(n)
    assert L.tlpk_ipm_get(kkt._h, _lib.IPM_THETA, pd(th), n) == _lib.OK
    assert np.isfinite(th).all() and (th >= 0).all()
    assert batch_reference(A, perm, ro, co, th, gP, gD)[1] == -1
    plans = []
    for plan in BATCH_PLANS:
        rD = gD.copy()
        for k, where in plan:
            rD[k] = batch_plant(A, perm, ro, th, gP[k], k, where)
        fc, lp = batch_reference(A, perm, ro, co, th, gP, rD)
        want = {k: int(cols[k][0] if where == "first" else cols[k][-1]) for k, where in plan}
        assert fc.tolist() == [want.get(k, -1) for k in range(3)] and lp == min(want, key=want.get), (plan, fc, lp)
        plans.append((int(fc[fc >= 0].min()), plan, rD, fc, lp))
    for _, plan, rD, fc, lp in sorted(plans, key=lambda p: (len(p[1]), p[0])):      # (ascending: a stale smaller column would win the min)
        fail.value = -7
        rc = L.tlpk_ipm_batch_factor(kkt._h, pu8(ones), pd(gP), pd(rD), C.byref(fail))
        rc2, got, nfail = each(kkt._h, ones, gP, rD)
        print(f"PVB plan {plan}: reference columns {fc.tolist()} LP {lp} | device *fail_lp {fail.value}, fail_col {got.tolist()}, nfail {nfail}")
        assert rc == _lib.NOT_POSDEF and fail.value == lp, (plan, fail.value, lp)
        assert rc2 == _lib.NOT_POSDEF and got.tolist() == fc.tolist() and nfail == len(plan), (plan, got, fc)
    rc2, got, nfail = each(kkt._h, ones, gP, gD)
    assert rc2 == _lib.OK and nfail == 0 and (got == -1).all()
    assert L.tlpk_ipm_batch_factor(kkt._h, pu8(ones), pd(gP), pd(gD), C.byref(fail)) == _lib.OK and fail.value == -1
    kkt.close()
