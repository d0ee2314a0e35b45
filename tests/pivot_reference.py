"""Reference for the verdict of a factorisation (include/tlpk.h: TLPK_NOT_POSDEF, tlpk_stats.fail_col = the permuted column of the first pivot that does
not carry the sign of its node), and the recipes that PLANT such a pivot at a chosen column.  Test infrastructure (plain numpy, long double): it takes
no code from the library and nothing from tests/emulate.py.  tests/test_pivot_verdict.py is the user; DESIGN.md section 1, "Pivot verdict sweep", has the arguments.

Reference.  d_0 .. d_{N-1} = the pivots of the L D L' of K^ without pivoting (backward_error.System: the handle's permuted matrix in long double, from the
double data the device forms).  They do not depend on any blocking.  The verdict is the first c with not (s_c d_c > 0): a pivot of the wrong sign, an
exact zero or a NaN (s = 1 for K1).

A plant that only moves the diagonal entry (c*, c*) of K^ by delta leaves d_0 .. d_{c*-1} as they are (the columns before c* in a postorder are
descendants of c* or lie in other subtrees, never ancestors) and makes d_{c*} + delta of d_{c*}: ONE factorisation per input and regime serves every
plant of that kind.  `planted_pivot` is that shortcut; tests/test_pivot_verdict.py holds it against a factorisation of the planted data.

Recipes (decisive in exact arithmetic, so that the reference alone decides; c* = permuted column, perm[c*] = its node):
  K1, row i                  regD[i] = -(A D A')_ii - 1: S_ii = -1, and a pivot never exceeds its diagonal entry: d <= -1.
  K2, constraint node n + i  regD[i] = -(A E^-1 A')_ii - 1, E = theta^-1 + Rp as passed: whatever correctly signed nodes went before,
                             d = Rd_i + a'(E + B' R^-1 B)^-1 a <= Rd_i + (A E^-1 A')_ii = -1.
  K2, variable node j        theta[j] = -(A' Rd^-1 A)_jj - regP[j] - 1: the mirror image, d >= +1 where a negative pivot is due.
  exact zero, K1, row i      theta[j] = +inf on every column j of row i (D_j = 1 / inf = 0), regD[i] = 0: row i of S is exactly zero in every order of
                             summation, row i of L stays zero, the pivot is 0.0 (this moves other rows too: its reference is a factorisation of its own).
  NaN, row / node            regD[i] = NaN (K2 variable node: theta[j] = NaN): only the diagonal entry (c*, c*) is NaN."""
import numpy as np
import scipy.sparse as sp

from backward_error import LD, U

MARGIN = 1e4                 # every pivot BEFORE a planted column: s_c d_c >= MARGIN N u F_cc (no rounding of any kernel can turn it)
DECISIVE = 0.5               # the planted pivot: wrong sign and |d| >= DECISIVE, or exactly 0.0, or NaN
PANEL = 48


def pivots_ld(system):
    """The pivots of the L D L' of system.K in long double: right-looking, no pivot replaced (the entries behind a zero or NaN pivot are not meaningful, those
    before it are).  Column by column inside a panel of PANEL columns, on the rows that hold a nonzero there; the rows behind the panel take the panel's
    update as one product.  The pivots do not depend on the panel width (d_j = K_jj - sum_k L_jk^2 d_k in any bracketing, to the last bits of long double)."""
    S = np.tril(system.K).astype(LD)
    S = S + np.tril(S, -1).T
    N = system.N
    d = np.zeros(N, LD)
    with np.errstate(all="ignore"):
        for c0 in range(0, N, PANEL):
            c1 = min(N, c0 + PANEL)
            w = c1 - c0
            below = c1 + np.nonzero((S[c1:, c0:c1] != 0).any(axis=1))[0]
            P = S[np.concatenate([np.arange(c0, c1), below])][:, c0:c1]
            for j in range(w):
                d[c0 + j] = P[j, j]
                v = P[j + 1:, j].copy()
                P[j + 1:, j] = v / d[c0 + j]
                P[j + 1:, j + 1:] -= np.outer(P[j + 1:, j], v[: w - j - 1])
            if below.size:
                L = P[w:]
                S[np.ix_(below, below)] -= (L * d[c0:c1]) @ L.T
    return d


def verdict(sign, d):
    """The first column whose pivot does not carry its sign (wrong sign, 0.0, NaN); None: the matrix factorises"""
    with np.errstate(invalid="ignore"):
        bad = np.nonzero(~(np.asarray(sign) * d > 0))[0]
    return int(bad[0]) if bad.size else None


def margins(system, d):
    """s_c d_c / (N u F_cc) of every column, and its running minimum over the columns BEFORE each column (inf before column 0)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        mg = (system.sign * d).astype(np.float64) / (system.N * U * np.diag(system.F))
    mg = np.where(np.isnan(mg), -np.inf, mg)
    before = np.concatenate([[np.inf], np.minimum.accumulate(mg)[:-1]])
    return mg, before


def _diag_sums(A, w):
    """(A diag(w) A')_ii for every row i, in double"""
    A = sp.csr_matrix(A) if sp.issparse(A) else np.asarray(A)
    sq = A.multiply(A) if sp.issparse(A) else A * A
    return np.asarray(sq @ w).ravel()


def diag_sums(kind, A, data):
    """What the sign recipes need of the unplanted data: ((A D A')_ii for every row, (A' Rd^-1 A)_jj for every column (K2 only)), D = 1 / (theta^-1 + Rp)"""
    th, rp, rd = (np.asarray(v, dtype=np.float64) for v in data[:3])
    return _diag_sums(A, 1.0 / (th + rp)), (_diag_sums(A.T, 1.0 / rd) if kind == "k2" else None)


def plant(kind, A, data, node, what="sign", sums=None):
    """(theta, regP, regD) of `data` with a failure planted at `node` (K1: a row; K2: a variable j < n or a constraint n + i); what: sign | zero | nan;
    sums: diag_sums(kind, A, data) where a caller plants many nodes of one data set"""
    th, rp, rd = (np.array(v, dtype=np.float64) for v in data[:3])
    m, n = A.shape
    rows, cols_ = sums if sums is not None else (diag_sums(kind, A, data) if what == "sign" else (None, None))
    if kind == "k1":
        i = int(node)
        if what == "sign":
            rd[i] = -rows[i] - 1.0
        elif what == "nan":
            rd[i] = np.nan
        else:
            assert what == "zero"
            row = sp.csr_matrix(A)[i] if sp.issparse(A) else None
            cols = row.indices if row is not None else np.nonzero(np.asarray(A)[i])[0]
            th[cols] = np.inf
            rd[i] = 0.0
        return th, rp, rd
    assert kind == "k2" and what in ("sign", "nan")
    if node >= n:
        i = int(node) - n
        rd[i] = np.nan if what == "nan" else -rows[i] - 1.0
    else:
        j = int(node)
        th[j] = np.nan if what == "nan" else -cols_[j] - rp[j] - 1.0
    return th, rp, rd


def planted_pivot(system, d, c, planted):
    """d_{c} of the data `planted` = plant(..., node perm[c], "sign" | "nan") from the pivots d of the unplanted system: d_c + (K^_cc planted - K^_cc),
    the difference of the two diagonal entries in long double as System forms them (K1, K2 constraint: Rd_i; K2 variable: -fl(theta^-1 + Rp))."""
    th0, rp0, rd0 = system.data[:3]
    th1, rp1, rd1 = planted
    node = int(system.perm[c])
    if system.kind == "k1":
        delta = LD(rd1[node]) - LD(rd0[node])
    elif node >= system.n:
        delta = LD(rd1[node - system.n]) - LD(rd0[node - system.n])
    else:
        delta = -(LD(th1[node] + rp1[node]) - LD(th0[node] + rp0[node]))
    return d[c] + delta


def decisive(sign_c, dc):
    """The planted pivot decides by itself: wrong sign by at least DECISIVE, or exactly zero, or NaN"""
    dc = LD(dc)
    return bool(np.isnan(dc) or dc == 0 or sign_c * dc <= -DECISIVE)


def offsets(ns, regime):
    """The offsets planted in a front of ns pivot columns.  ones: {0, 1, ns - 1} and every o with o mod 16 in {0, 15} -- the panel cut of the 16-column
    panels, the 64-column blocks, the 256-column block columns, the last column of every partial block.  mid: {0, 15, 16, 63, 64, ns - 1}."""
    if regime == "ones":
        out = {0, 1, ns - 1} | {o for o in range(ns) if o % 16 in (0, 15)}
    else:
        out = {0, 15, 16, 63, 64, ns - 1}
    return sorted(o for o in out if 0 <= o < ns)


def planted_columns(kkt, regime):
    """Ascending permuted columns of the sweep for a handle: offsets() of every analysed front (every isolated 1 x 1 front is a front of one column)"""
    col0, ns = kkt.symbolic("front_col0"), kkt.symbolic("front_ns")
    return sorted({int(c) + o for c, w in zip(col0.tolist(), ns.tolist()) for o in offsets(int(w), regime)})
