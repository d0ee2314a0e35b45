"""Dense-handle shape sweep: a dense matrix on either side of every cut at which the kernels of dense_kernels.hip change behaviour -- the 128 x 128
tile of k_dense_syrk and its 64-row wave quarters, the K parts of the split SYRK (analyse_dense_matrix: `split` parts of `kc` columns, kc a multiple of the
16-column slab) with a last part of one column, of 16 k + 1 columns and of whole slabs, the unpadded panel below 64 rows, n = 0, 1, 2, the 512-row
workgroup and the column chunks of k_dense_gemv_n, the four waves, the row pairs and the lane loop of k_dense_gemv_t -- checked with the criterion of
tests/test_backward_error.py: componentwise backward error against long double, omega_hard <= 1 and omega_unit <= 8 max(restatement's, 1), dx entry by
entry against the device's own dy (k_dense_gemv_t), the right-hand side's allowance inside the solve bound (k_dense_gemv_n).  No tolerance of its own.

Which cut a shape sits on is decided by analyse_dense_matrix; the handle exports it as tlpk_symbolic_get(h, "dense_geometry") = (split, kc, chunks, cw,
dense_lda, panel lda), the numbers the kernels receive.  The table below is asserted against those numbers (test_the_sweep_holds_every_cut), the rule itself
against a plain restatement over a grid of shapes (test_geometry_rule_*).  Every input keeps m <= 1100 (the long-double residual covers every row) and
m m n / 2 <= 1.5e8 long-double multiply-adds for K^ (a condition of the table, asserted; the largest, 1025 x 200, has 1.05e8).

CPU: the table; the rule; per input and regime the restatement (the guard of the inputs) and the emulator that forms S the way the device does FROM THE
EXPORTED GEOMETRY (ShapeEmulator); the mutants planted in that emulator.  GPU (-m gpu): the device leg per input and regime, the mid one factorising its data
over the ones factor in NaN-poisoned storage; a pair of right-hand sides (NR = 2 of both GEMVs) bit for bit two single solves; two updates bit for bit, the
panel's padding rows exact zeros; n = 0.  The table of a run on an MI355X is profiles/dense_shape_sweep.txt.

What is left out, and why.
  * Regime late (theta over 16 decades, 5 % exact zeros, regularisations sqrt(eps)) runs only where the restatement factorises it: LATE, chosen on the CPU.
    A D A' has rank <= n and the regularisation is sqrt(eps), so no input with n < m is a candidate (tests/test_front_shapes.py: a negative pivot on each of
    its ten); of those with n >= m the restatement factorises all but 513 x 529 (NOT_LATE: n barely above m, a negative pivot at column 505).
  * The mutation leg of tests/test_backward_error.py (one small entry of L or w moved by 1e-9) is not run: on a dense K^ every row is full and the allowance of
    a row sums over all m entries -- tests/test_front_shapes.py shows that the leg is a coin toss there.  The mutants of this file are planted in the SYRK
    instead (MUTATIONS), which is where this sweep looks.
  * 513 x 4097 (a last part of one column under 15 tiles) has 5.4e8 multiply-adds: over the cap.  129 x 321 and 193 x 321 hold that cut."""
import numpy as np
import pytest

import tulip_jl_amd as tk
from backward_error import Allowances, dense_L_of_emulator, solve_stats
from emulate import panels_to_dense_L, pk_off
from helpers import DevBuf, ipm_like_data
from test_backward_error import RATIO, SEED, Problem, device_leg
from test_dense_backend import DenseEmulator, create_raw, dense_A
from test_front_shapes import with_rhs
from tulip_jl_amd import _lib

TILE, SLAB, GEMV_ROWS = 128, 16, 512          # dense_kernels.hip / tlpk_host.hpp: TILE, DS_KT, DGEMV_ROWS
MAX_MADDS, MAX_M = 1.5e8, 1100

# name -> (m, n), named for the cut.  The comments give (split x kc | chunks x cw) as exported.
SHAPES = {
    # SYRK unsplit, one partly empty tile; the panel is unpadded below 64 rows (plda = m < dense_lda); n = 0, 1, 2: no slab / one staging half / both
    "m1_n0": (1, 0),                      # 1 x 16 | 1 x 1   no column at all: S = Rd, dx empty
    "m2_n1": (2, 1),                      # m <= 2 for k_dense_gemv_t; only sk0 = 0 stages a real column
    "m17_n2": (17, 2),                    # n mod 4 = 2
    "m63_n17": (63, 17),                  # 1 x 32 | 2 x 9   one slab + 1; plda = 63 under dense_lda = 64
    "m64_n1": (64, 1),                    # the first padded panel (plda = 64)
    "m65_n0": (65, 0),                    # n = 0 above 64 rows: 15 padding rows
    "m127_n19": (127, 19),                # 1 x 32 | 2 x 10  n mod 4 = 3; odd m below 128
    # SYRK split, ONE tile: m <= 128 from n = 768
    "m1_split": (1, 769),                 # 10 x 80 | 49 x 16   last part 49 = 3 slabs + 1
    "m63_split": (63, 769),               # the same over an unpadded panel: syrk_store's row >= plda
    "m64_parts64": (64, 768),             # 12 x 64: parts of exactly 64 columns, the floor of the rule
    "m128_split": (128, 785),             # 10 x 80, last part 65 = 4 slabs + 1; the full tile
    # SYRK split, several tiles at a tile edge
    "m129_slabs": (129, 320),             # 5 x 64: every part whole slabs
    "m129_last1": (129, 321),             # 5 x 80: last part ONE column
    "m130_last17": (130, 337),            # 5 x 80: last part 17 = one slab + 1; 14 padding rows; even m above 128
    "m130_view": (130, 337),              # the same created from a view into a taller array (lda = 141 > m) whose rows beyond m are NaN
    "m193_last1": (193, 321),             # 5 x 80: the wave-row boundary inside the second tile
    "m257_last40": (257, 200),            # 3 x 80: last part 40 = two slabs + 8
    "m513_split": (513, 529),             # 7 x 80, 15 tiles, last part 49; k_dense_gemv_n: second 512-row workgroup with 8 live threads
    # SYRK unsplit over several tiles, for contrast
    "m257_unsplit": (257, 100),           # 1 x 112 | 7 x 15
    # GEMV
    "m512_n17": (512, 17),                # one row block (dense_lda = 512), 2 chunks of 9 | 8
    "m513_n17": (513, 17),                # two row blocks (dense_lda = 528)
    "m1025_rows3": (1025, 200),           # three row blocks; 45 tiles x 3 parts
    "m16_cw17": (16, 16385),              # 964 chunks of 17, the last of 14: cw > 16 with a short last chunk; 54 parts of 304
    "m1_cw17": (1, 16385),
}
VIEW = {"m130_view": 11}                  # rows of NaN below the matrix in the caller's array


def _make(name):
    m, n = SHAPES[name]

    def make():
        A = dense_A(m, n, seed=m + n)
        if name in VIEW:
            big = np.full((m + VIEW[name], n), np.nan, order="F")
            big[:m] = A
            A = big[:m]
        return A, {}
    return make


INPUTS = {name: ("k1", "dense", _make(name)) for name in SHAPES}
# Regime late only where the restatement factorises it (module docstring).  NOT_LATE: n >= m, and the restatement meets a negative pivot.
LATE = ["m1_split", "m63_split", "m64_parts64", "m128_split", "m129_slabs", "m129_last1", "m130_last17", "m130_view", "m193_last1", "m16_cw17", "m1_cw17"]
NOT_LATE = ["m513_split"]                 # 513 x 529: pivot 505 is -1.3e-4
COMBOS = [(name, reg) for name in SHAPES for reg in ("ones", "mid")] + [(name, "late") for name in LATE]
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


# ---------------------------------------------------------------------------------------------------------------------------------
# the exported geometry and its restatement
# ---------------------------------------------------------------------------------------------------------------------------------
GEO = ("split", "kc", "chunks", "cw", "dlda", "plda")


def geometry(kkt):
    return dict(zip(GEO, (int(v) for v in kkt.symbolic("dense_geometry"))))


def cdiv(a, b):
    return -(-a // b)


def geometry_rule(m, n):
    """analyse_dense_matrix restated.  SYRK: the lower triangle has ntiles tiles, two workgroups per compute unit make rounds of 512; K = n is cut into the
    smallest number of parts that fills its rounds best (by 2 % or more over every smaller number), of at least 512 columns each (64 while everything is
    inside the first round), with at most 4096 raw tiles; kc = the part's width rounded up to whole slabs, and the number of parts again from kc.  GEMV:
    about 1024 workgroups = row blocks x chunks, a chunk no narrower than a slab's 16 columns wherever n allows; cw from the chunks, the chunks from cw, and cw
    once more from the chunks that are kept."""
    T = cdiv(m, TILE)
    ntiles = T * (T + 1) // 2
    fill = lambda s: (ntiles * s) / (cdiv(ntiles * s, 512) * 512)      # noqa: E731
    split, best = 1, fill(1)
    s = 2
    while s <= 64 and ntiles * s <= 4096:
        if n // s < (64 if ntiles * s <= 512 else 512):
            break
        if fill(s) >= best + 0.02:
            best, split = fill(s), s
        s += 1
    kc = max(SLAB, cdiv(cdiv(n, split), SLAB) * SLAB)
    split = max(1, cdiv(n, kc))
    dlda = cdiv(m, 16) * 16
    chunks = max(1, min(1024 // cdiv(dlda, GEMV_ROWS), cdiv(n, 16)))
    cw = max(1, cdiv(n, chunks))
    chunks = max(1, cdiv(n, cw))
    cw = max(1, cdiv(n, chunks))
    return dict(split=split, kc=kc, chunks=chunks, cw=cw, dlda=dlda, plda=dlda if m >= 64 else m), (ntiles * split * TILE * TILE if split > 1 else 0)


GRID_M = sorted({1, 2, 15, 16, 17, 63, 64, 65, 193, 1100, 4200} | {TILE * k + d for k in (1, 2, 3, 4, 5, 6, 8, 12, 16, 24, 32) for d in (-1, 0, 1)})
GRID_N = sorted({0, 1, 2, 337, 785, 19999, 20000} | {SLAB * k + d for d in (-1, 0, 1) for k in
                                                    [1, 2, 4, 5, 8, 20, 21, 32, 48, 49, 64, 96, 128, 160, 192, 256, 320, 384, 512, 640, 768, 1024, 1100, 1249]
                                                    + list(range(3, 1250, 61))})          # about 6000 analyse-only handles: a second or two
_grid = {}


def grid():
    """(m, n) -> (exported geometry, spart_len) of an analyse-only handle.  The matrix is never read by such a handle: one untouched buffer serves them all."""
    if not _grid:
        buf = np.empty(max(GRID_M) * max(GRID_N), order="F")
        L = _lib.lib()
        for m in GRID_M:
            for n in GRID_N:
                rc, h, msg = create_raw(m, n, buf, m)
                assert rc == _lib.OK, (m, n, msg)
                g = dict(zip(GEO, (int(v) for v in _lib.symbolic_array(h, "dense_geometry"))))
                _grid[(m, n)] = (g, int(_lib.symbolic_array(h, "singles")[-1]), int(_lib.symbolic_array(h, "front_lda")[0]))
                L.tlpk_destroy(h)
    return _grid


def test_geometry_rule_is_the_restated_one():
    for (m, n), (g, spart, front_lda) in grid().items():
        want, slots = geometry_rule(m, n)
        assert g == want, (m, n, g, want)
        assert g["plda"] == front_lda and spart >= slots, (m, n)
    assert any(g["split"] > 1 for g, _, _ in grid().values()) and any(g["cw"] > 16 for g, _, _ in grid().values())


def test_geometry_rule_keeps_what_the_kernels_rely_on():
    for (m, n), (g, spart, _) in grid().items():
        T = cdiv(m, TILE)
        ntiles = T * (T + 1) // 2
        split, kc, chunks, cw = g["split"], g["kc"], g["chunks"], g["cw"]
        assert kc % SLAB == 0 and kc >= SLAB and split >= 1 and chunks >= 1 and cw >= 1, (m, n, g)
        assert g["dlda"] % 16 == 0 and m <= g["dlda"] < m + 16 and g["plda"] in (m, g["dlda"]), (m, n, g)
        if n > 0:
            assert (split - 1) * kc < n <= split * kc, (m, n, g)               # no empty part, no column left out
            assert (chunks - 1) * cw < n <= chunks * cw, (m, n, g)             # no empty chunk, no column left out
        else:
            assert (split, chunks) == (1, 1), (m, n, g)
        if split > 1:
            assert ntiles * split <= 4096 and spart >= ntiles * split * TILE * TILE, (m, n, g, spart)      # slot = tile * split + part
        assert chunks * cdiv(g["dlda"], GEMV_ROWS) <= 1024, (m, n, g)                # the grid of k_dense_gemv_n


def test_sparse_handles_report_no_dense_geometry():
    from helpers import random_lp_matrix
    A = random_lp_matrix(30, 50, 3, 1)
    for system in (tk.K1(), tk.K2()):
        assert tk.setup(A, system, tk.Backend(device=-1)).symbolic("dense_geometry").tolist() == [0] * 6


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the table holds every cut
# ---------------------------------------------------------------------------------------------------------------------------------
_geo = {}


def cuts_of(names):
    """The set of cuts that the inputs `names` sit on, from the EXPORTED geometry of their analyse-only handles."""
    have = set()
    for name in names:
        m, n = SHAPES[name]
        if name not in _geo:
            _geo[name] = geometry(tk.setup(INPUTS[name][2]()[0], tk.K1(), tk.DenseBackend(device=-1)))
            g = _geo[name]
            print(f"GEO {name:15s} {m:5d} x {n:5d} | syrk {g['split']:2d} x {g['kc']:3d} | gemv_n {g['chunks']:3d} x {g['cw']:2d} | dense_lda {g['dlda']:4d} panel lda {g['plda']:4d}")
        g = _geo[name]
        T = cdiv(m, TILE)
        last = n - (g["split"] - 1) * g["kc"]                     # columns of the last K part
        if g["split"] == 1:
            have.add(("unsplit", "m", m)); have.add(("unsplit", "n", n))
            if n == 0:
                have.add(("unsplit n=0", "m <= 64" if m <= 64 else "m > 64"))
            if T > 1:
                have.add("unsplit, several tiles")
        else:
            have.add(("split", "one tile" if T == 1 else "several tiles", m))
            if T == 1 and m < 64:
                have.add("split, unpadded panel")
            if T == 1 and g["kc"] == 64 and last == 64:
                have.add("split, parts of exactly 64")
            if T > 1:
                have.add(("split, several tiles, last part", "1" if last == 1 else "16k+1" if last % SLAB == 1 else "slabs" if last % SLAB == 0 else "slabs+r"))
                if g["plda"] > m:
                    have.add("split, padding rows")
            if name in VIEW:
                have.add("split, lda > m at create")
        rb = cdiv(g["dlda"], GEMV_ROWS)
        have.add(("gemv_n row blocks", min(rb, 3)))
        if rb == 2 and g["dlda"] - GEMV_ROWS < 2 * 64:
            have.add("gemv_n second row block under one wave")
        if g["dlda"] == GEMV_ROWS:
            have.add("gemv_n one full row block")
        if g["cw"] > 16 and n % g["cw"] != 0:
            have.add(("gemv_n cw > 16, short last chunk", "m = 1" if m == 1 else "m > 1"))
        if g["cw"] % 4:
            have.add("gemv_n cw not a multiple of the unroll")
        if g["chunks"] == 2 and n == 17 and g["cw"] == 9:
            have.add(("gemv_n 2 chunks of 9 | 8", m))
        have.add(("gemv_t n mod 4", n % 4))
        have.add(("gemv_t m", "odd" if m % 2 else "even", "<= 128" if m <= 128 else "> 128"))
        if m <= 2:
            have.add(("gemv_t m <= 2", m))
    return have


WANTED = ([("unsplit", "m", m) for m in (1, 2, 17, 63, 64, 65)] + [("unsplit", "n", n) for n in (0, 1, 2, 17)]
          + [("unsplit n=0", "m <= 64"), ("unsplit n=0", "m > 64"), "unsplit, several tiles"]
          + [("split", "one tile", m) for m in (1, 63, 64, 128)] + ["split, unpadded panel", "split, parts of exactly 64"]
          + [("split", "several tiles", m) for m in (129, 130, 193, 257, 513)]
          + [("split, several tiles, last part", k) for k in ("1", "16k+1", "slabs", "slabs+r")] + ["split, padding rows", "split, lda > m at create"]
          + [("gemv_n row blocks", k) for k in (1, 2, 3)] + ["gemv_n second row block under one wave", "gemv_n one full row block"]
          + [("gemv_n cw > 16, short last chunk", k) for k in ("m = 1", "m > 1")] + ["gemv_n cw not a multiple of the unroll"]
          + [("gemv_n 2 chunks of 9 | 8", m) for m in (512, 513)]
          + [("gemv_t n mod 4", k) for k in (0, 1, 2, 3)] + [("gemv_t m", a, b) for a in ("odd", "even") for b in ("<= 128", "> 128")]
          + [("gemv_t m <= 2", m) for m in (1, 2)])


def missing_cuts(without=()):
    have = cuts_of([name for name in SHAPES if name not in without])
    return [c for c in WANTED if c not in have]


def test_the_sweep_holds_every_cut():
    assert missing_cuts() == []
    for name, (m, n) in SHAPES.items():
        assert m <= MAX_M and m * m * n / 2 <= MAX_MADDS, name
    assert set(LATE) | set(NOT_LATE) == {name for name, (m, n) in SHAPES.items() if n >= m}
    # (the test has teeth: each of these is the only carrier of a cut)
    assert missing_cuts(without=["m129_last1", "m193_last1"]) == [("split", "several tiles", 193), ("split, several tiles, last part", "1")]
    assert missing_cuts(without=["m64_parts64"]) == [("split", "one tile", 64), "split, parts of exactly 64"]
    assert missing_cuts(without=["m16_cw17"]) == [("gemv_n cw > 16, short last chunk", "m > 1")]


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the emulator that forms S from the exported geometry
# ---------------------------------------------------------------------------------------------------------------------------------
class ShapeEmulator(DenseEmulator):
    """tests/test_dense_backend.py's DenseEmulator with k_dense_syrk / k_dense_syrk_reduce restated from the exported geometry: per 128 x 128 tile of the
    lower triangle and per K part a raw tile, accumulated slab by slab (16 columns) in chunks of four columns (one v_mfma_f64_16x16x4_f64 per chunk), the
    operand rows beyond the last row of the device copy clamped to it, D applied to the column operand; split > 1: the raw tiles of a tile added in part
    order where row >= col, row < m, col < m, zero elsewhere; then syrk_store: + regD on the diagonal, exact zeros on the padding rows m .. plda - 1 and
    above the diagonal inside the column's 64-column slice, nothing above that slice and nothing from row plda on.  All other storage stays NaN.
    `mut` plants one of MUTATIONS."""

    def __init__(self, kkt, mut=None):
        super().__init__(kkt)
        self.geo, self.mut = geometry(kkt), mut

    def form_panel(self, A):
        m, n = A.shape
        g, mut = self.geo, self.mut
        split, kc, dlda, plda, loff = g["split"], g["kc"], g["dlda"], g["plda"], int(self.loff[0])
        assert plda == int(self.lda[0])
        dA = np.zeros((dlda, n)); dA[:m] = A                                       # the device copy: padding rows zero
        clamp = m - 2 if mut == "clamped_row" else dlda - 1
        T = cdiv(m, TILE)
        r128 = np.arange(TILE)
        for ti in range(T):
            for tj in range(ti + 1):
                i0, j0 = ti * TILE, tj * TILE
                Ai, Aj = dA[np.minimum(i0 + r128, clamp)], dA[np.minimum(j0 + r128, clamp)]
                parts = []
                for p in range(split):
                    k_lo = p * kc
                    kw = max(0, min(n, k_lo + kc) - k_lo)
                    if mut == "last_column" and p == split - 1:
                        kw -= 1
                    Dp = self.D[:kw] if (mut == "part_offset" and p > 0) else self.D[k_lo: k_lo + kw]
                    Bj = Aj[:, k_lo: k_lo + kw] * Dp[None, :]                      # pb = A[rb, k] D[k]: one rounding
                    acc = np.zeros((TILE, TILE))
                    for k4 in range(0, kw, 4):                                     # (the zero columns that fill a slab's tail add exact zeros)
                        acc += Ai[:, k_lo + k4: k_lo + min(k4 + 4, kw)] @ Bj[:, k4: k4 + 4].T
                    parts.append(acc)
                if split > 1:
                    live = ((i0 + r128)[:, None] >= (j0 + r128)[None, :]) & ((i0 + r128)[:, None] < m) & ((j0 + r128)[None, :] < m)
                    S = parts[0].copy()
                    for p in range(1, split - 1 if mut == "last_part" else split):
                        S += parts[p]
                    S = np.where(live, S, 0.0)
                else:
                    S = parts[0]
                for c in range(j0, min(j0 + TILE, m)):                             # syrk_store
                    lo, hi = max(i0, (c >> 6) << 6), min(i0 + TILE, plda)
                    if hi <= lo:
                        continue
                    r = np.arange(lo, hi)
                    v = S[r - i0, c - j0].copy()
                    v[(r < c) | (r >= m)] = 0.0
                    if mut == "padding_row":
                        v[r == m] = 1.0
                    if lo <= c < hi and not (mut == "regD_last_row" and c == m - 1):
                        v[c - lo] += self.regD[c]
                    self.Lval[loff + pk_off(plda, c) + r] = v
        return None


def padding_rows(lval, loff, m, plda):
    """The stored entries of the rows m .. plda - 1 of a panel (k_dense_syrk writes exact zeros there and the factorisation keeps them)."""
    if plda == m:
        return np.zeros(0)
    return np.concatenate([lval[loff + pk_off(plda, c) + m: loff + pk_off(plda, c) + plda] for c in range(m)])


def shape_emulator_leg(pb, mut=None):
    pb.assert_good_input()
    em = ShapeEmulator(pb.kkt, mut)
    em.update(*pb.data[:3])
    pad = padding_rows(em.Lval, int(em.loff[0]), em.m, em.geo["plda"])
    if em.fail_col is not None:
        return dict(factor=dict(hard=np.inf, unit=np.inf, at=em.fail_col)), pad
    return pb.check("emulator" if mut is None else mut[:11], dense_L_of_emulator(em, pb.system.N)), pad


def test_restatement_is_inside_the_bound(pb):
    pb.assert_good_input()


def test_emulated_tiles_and_parts_are_inside_the_bound(pb):
    """Ties the exported geometry to the criterion: a part rule that lost a column, doubled one or mis-sized the last part would show here."""
    st, pad = shape_emulator_leg(pb)
    assert st["factor"]["hard"] <= 1.0, st
    assert st["factor"]["unit"] <= RATIO * max(pb.stats["factor"]["unit"], 1.0), (st, pb.stats)
    assert not pad.any()


def test_late_data_is_used_where_the_restatement_factorises_it():
    """The input with n >= m that is left out of LATE, and one with n < m: the restatement meets a negative pivot there, so the regime is no test input (and
    would be a FAILURE of test_restatement_is_inside_the_bound, not a skip, were it listed)."""
    for name in ("m513_split", "m257_last40"):
        assert name not in LATE
        p = Problem(name, "late", INPUTS)
        assert "error" in p.stats and p.L is None, name


# mutant -> (input, what it is).  Each must push the factor's omega_hard above 1 in regime mid (regime ones has D = 1/2 throughout: "part_offset" changes
# nothing there, by construction).  "padding_row" is the exception: see its test.
MUTATIONS = {
    "last_column": ("m129_last1", "the last column of the last K part is dropped (there: the whole part, one column)"),
    "part_offset": ("m129_last1", "D is indexed without the part's offset for the parts after the first"),
    "last_part": ("m129_last1", "the reduction leaves out the last part"),
    "regD_last_row": ("m130_last17", "regD is not added on row m - 1"),
    "clamped_row": ("m129_last1", "the operand rows are clamped one row early: row 128 of 129 reads row 127's data into stored entries"),
}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_mutant_breaks_the_bound(mut):
    pb = problem(MUTATIONS[mut][0], "mid")
    good, _ = shape_emulator_leg(pb)
    bad, _ = shape_emulator_leg(pb, mut)
    print(f"MUT {mut:14s} on {pb.name}: omega_hard {good['factor']['hard']:.3e} -> {bad['factor']['hard']:.3e}")
    assert good["factor"]["hard"] <= 1.0 < bad["factor"]["hard"]


def test_mutant_padding_row_is_seen_in_the_storage_only():
    """A padding row (row m of the panel, m < plda) given a non-zero value.  The criterion is blind to it AT ANY SHAPE, not only at this one: no kernel of
    the factorisation carries a padding row into a row of L (the rows below a diagonal block are independent of each other in k_trsm and as operand rows
    of the updates), and L is all the criterion sees -- omega_hard does not move by a bit.  No input can change that, so the zeros are asserted where they
    are: padding_rows() on the emulator's storage here, and on the device's panels in test_device_two_updates_*."""
    pb = problem("m130_last17", "mid")
    good, pad0 = shape_emulator_leg(pb)
    bad, pad1 = shape_emulator_leg(pb, "padding_row")
    print(f"MUT padding_row    on {pb.name}: omega_hard {good['factor']['hard']:.3e} -> {bad['factor']['hard']:.3e}; non-zero padding entries {np.count_nonzero(pad0)} -> {np.count_nonzero(pad1)}")
    assert bad["factor"]["hard"] == good["factor"]["hard"] <= 1.0
    assert pad0.size == 130 * 14 and not pad0.any() and np.count_nonzero(pad1) == 130


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def device_handle(pb):
    kkt = tk.setup(INPUTS[pb.name][2]()[0], tk.K1(), tk.DenseBackend(device=0))
    assert geometry(kkt) == geometry(pb.kkt)                      # the device handle is launched with the numbers the table was checked against
    return kkt


@pytest.mark.gpu
def test_device_factor_and_solves_are_inside_the_bound(pb, monkeypatch):
    """The device leg of tests/test_backward_error.py.  The leg of regime mid is the one with stale storage: TLPK_POISON=1 (the factor storage starts as
    NaNs), the ones data factorised first, then the mid data on the same handle."""
    if pb.regime != "mid":
        return device_leg(pb)
    monkeypatch.setenv("TLPK_POISON", "1")
    m, n = pb.A.shape
    device_leg(pb, who="device+stale", first=ipm_like_data(m, n, SEED, "ones")[:3])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_device_pair_of_right_hand_sides(name):
    """tlpk_solve2_device (NR = 2 of k_dense_gemv_n and k_dense_gemv_t): both solutions bit for bit those of two single device-pointer solves, and both
    inside the solve bound of the device's own factor, dx entry by entry against the device's dy."""
    from backward_error import dx_stats
    pb = problem(name, "mid")
    pb.assert_good_input()
    kkt = device_handle(pb)
    th, rp, rd, xp, xd = pb.data
    m, n = pb.A.shape
    rhs = [(xp, xd), (xp[::-1].copy(), xd[::-1].copy())]
    tk.update(kkt, th, rp, rd)
    d = [DevBuf(v) for v in (rhs[0][0], rhs[0][1], rhs[1][0], rhs[1][1])]
    s = [DevBuf(sz, np.nan) for sz in (n, m, n, m)]
    kkt.solve_device(s[0].ptr, s[1].ptr, d[0].ptr, d[1].ptr)
    kkt.solve_device(s[2].ptr, s[3].ptr, d[2].ptr, d[3].ptr)
    single = [(s[0].get(), s[1].get()), (s[2].get(), s[3].get())]
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
        x = dx_stats(sysk, dx, dy)
        print(f"BE {name:15s} mid   pair rhs {k}  N={sysk.N:5d} | solve hard={v['hard']:.3e} unit={v['unit']:.3e} | dx hard={x['hard']:.3e} unit={x['unit']:.3e}")
        assert v["hard"] <= 1.0, f"{name} rhs {k}: omega_hard = {v['hard']:.3e} at {v['at']}"
        assert v["unit"] <= RATIO * max(ref, 1.0), f"{name} rhs {k}: omega_unit = {v['unit']:.3e}, the restatement's {ref:.3e}"
        assert x["hard"] <= 1.0, f"{name} rhs {k}: dx omega_hard = {x['hard']:.3e} at {x['at']}"
        assert x["unit"] <= RATIO * max(pb.stats["dx"]["unit"], 1.0), f"{name} rhs {k}: dx omega_unit = {x['unit']:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_device_two_updates_give_the_same_panels(name, monkeypatch):
    """The reduction adds the parts in part order, whatever order they were computed in: two updates with the same data give the same bits -- in storage that
    started as NaNs, and with exact zeros in the panel's padding rows."""
    monkeypatch.setenv("TLPK_POISON", "1")
    pb = problem(name, "mid")
    kkt = device_handle(pb)
    th, rp, rd = pb.data[:3]
    tk.update(kkt, th, rp, rd); p0 = kkt.factor_panels().copy()
    tk.update(kkt, th, rp, rd); p1 = kkt.factor_panels().copy()
    m, plda, loff = pb.A.shape[0], geometry(kkt)["plda"], int(kkt.symbolic("front_loff")[0])
    kkt.close()
    pad = padding_rows(p1, loff, m, plda)
    print(f"PAD {name:15s} {pad.size} padding entries, {np.count_nonzero(pad)} non-zero, {np.count_nonzero(np.isnan(pad))} NaN")
    assert p0.tobytes() == p1.tobytes()
    assert np.isfinite(np.tril(panels_to_dense_L(pb.kkt, p1))).all()
    assert pad.size == m * (plda - m) and not pad.any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["m1_n0", "m65_n0"])
def test_device_without_columns(name):
    """n = 0: no slab (S = Rd), no chunk, no column of dx.  The update succeeds, dy = xi_p / Rd inside the solve bound, dx is empty -- and so the second time."""
    pb = problem(name, "mid")
    pb.assert_good_input()
    m, n = pb.A.shape
    assert n == 0
    kkt = device_handle(pb)
    th, rp, rd, xp, xd = pb.data
    for it in range(2):
        tk.update(kkt, th, rp, rd)
        dx = np.zeros(0); dy = np.full(m, np.nan)
        tk.solve(dx, dy, kkt, xp, xd)
        L = np.tril(panels_to_dense_L(kkt, kkt.factor_panels()))
        st = pb.check(f"device n=0 #{it}", L, dxdy=(dx, dy))
        assert dx.size == 0
        for part, v in st.items():
            assert v["hard"] <= 1.0, f"{name} {part}: omega_hard = {v['hard']:.3e} at {v['at']}"
            assert v["unit"] <= RATIO * max(pb.stats[part]["unit"], 1.0), f"{name} {part}: omega_unit = {v['unit']:.3e}"
    kkt.close()
