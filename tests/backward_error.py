"""Componentwise backward error of a factor P K P' = L S L' and of the solves through it.  Test infrastructure (plain numpy): never
imported by the product.  This docstring is the specification of the bounds tests/test_backward_error.py asserts.

Notation.  u = 2^-53.  N = order of the factored matrix (m for K1, n + m for K2, m + k with k dense columns).  K^ = that matrix in the
handle's permuted numbering, built HERE in long double (64-bit significand) from A, theta^-1, Rp, Rd and the DOUBLE values D the device
forms (K1: D = fl(1 / fl(theta^-1 + Rp)); K2 and the dense nodes: fl(theta^-1 + Rp)).  S = diag(+-1) (I for K1; -1 on the variable
nodes of K2 and on the dense nodes).  F = the matrix of the absolute values of the terms of K^ (K1: |A| D |A|' + |Rd|; K2: |K^|),
p_ij = the number of terms of entry (i, j).  The columns are cut into the diagonal blocks b the device inverts: for every front,
col0 + 64 k, width min(64, ns - 64 k) (tlpk_host.hpp: NB_IN = 64).  L_bb = the diagonal block, X_b = its inverse (long double here),
M_b = |L_bb| |X_b| (entrywise >= I), M16_b = the same product over the 16 x 16 diagonal sub-blocks of the block alone (>= I, <= M_b).

Evaluation.  A dot product of length t in long double is off by at most t 2^-64 = (t 2^-11) u times its absolute terms: N / 2048 (p / 2048
for the terms of K^) is added to every coefficient below.  Only the residuals are evaluated in long double; the allowances are products
of non-negative doubles (relative error ~ N u, irrelevant).

FACTOR.  R = |K^ - L S L'| on the lower triangle, entry by entry, against

  (p + 3) u E_form,   E_form = F.   The device sums p_ij terms fl(fl(a_ik a_jk) D_k) (the pair products come from the host, one rounding; one for
        the product with D) with p_ij - 1 additions and one more for Rd: p + 2 roundings on any term, in any order -- the sparse assembly
        (k_assemble, k_front_assemble), the split-K SYRK of the dense handle with its reduction, all alike.  The coefficient is p + 3: one to spare.
  (N + 1 + 4) u E_chol,   E_chol = |L| |L'|.   Higham, Accuracy and Stability, Thm 10.3 (gamma_{N+1}; any order of summation: an entry is a sum of
        its assembled value and at most N - 1 products, however the terms are bracketed -- left-looking, right-looking, split-K parts,
        update matrices passed up by extend-add: a sum of T terms has T - 1 additions in all, so no term passes through more).  The
        theorem counts ONE rounding each for the square root and for the division by it.  The device forms isq ~ |d|^-1/2 by the hardware
        estimate and two Newton steps, L_jj = d isq with one correction step, L_ij = a_ij isq (potrf_block, dpp_panel, k_potrf_small): at
        most 4 roundings more than the theorem's two on the path of an entry.  This is the design's documented rsq + Newton square root:
        its term is 4 u E_chol.
  128 u E_inv,   E_inv[i, b] = |L[i, b]| |L_bb'| M_b'   (rows i below block b, zero elsewhere), and
  96 u E_inv2,  E_inv2[i, b] = |L[i, b]| |L_bb'| M_b' M16_b'.   The rows below a diagonal block are PRODUCTS with its explicit inverse:
        L_21 = fl(S_21 X^_b') S_bb (k_trsm, k_trsm_thin, the in-block solves of k_potrf_wide, the strip role of k_chain), where S_21 is the
        block after the updates by the block columns to its left (those are E_chol's).  Which residual does X^_b satisfy?
          * potrf_block, k_potrf_small: the row eliminations of the block applied to an identity = forward substitution for the columns of
            the inverse, then the row scaling: |L_bb X^_b - I| <= gamma_64 |L_bb| |X^_b| (Higham 14.2, Method 1) -- a RIGHT residual.
            The multipliers are fl(a_rj inv2) with inv2 = isq^2, not L_rj / L_jj: <= 8 u more, relative.
          * potrf_block_dpp (the default diagonal block since round 5): 16 x 16 diagonal sub-blocks inverted by forward substitution, the
            sub-blocks below them as W_ij = -W_ii G_ij, G_ij = sum_k L_ik W_kj on the matrix cores.  Then, for i > j,
            (L X^)_ij = -E_ii G_ij + L_ii D1 - D2 with |E_ii| <= gamma_16 |L_ii||X_ii|, |D1| <= gamma_16 |X_ii||G_ij|, |D2| <= gamma_48 (|L||X|)_ij
            and |G_ij| <= (|L||X|)_ij: |L_bb X^_b - I| <= gamma_80 M16_b M_b.  Still a right residual, with ONE MORE FACTOR M16_b.
        M16_b M_b >= M_b covers both: L_bb X^_b = I + E, |E| <= 96 u M16_b M_b (80 + 8 and slack for X^ in place of X, first order).  The
        product rounds as L_21 = S_21 X^_b' + d, |d| <= gamma_64 |S_21| |X_b'|, and S_21 = (L_21 - d) X^_b^-T = L_21 L_bb' to first order, so
          L_21 L_bb' - S_21 = S_21 E' + d L_bb',     |.| <= |L_21| |L_bb'| (96 (M16_b M_b)' + 64 M_b') u
        (the signs S_bb are exact): 128 E_inv -- the term of a plain right residual, gamma_64 for the product and as much again for the
        inverse, which is to spare here -- and 96 E_inv2, which carries the inverse's residual with the factor M16_b of potrf_block_dpp.

  omega_hard = max R / (u [(p + 3) E_form + (N + 5) E_chol + 128 E_inv + 96 E_inv2])   must be <= 1: the theorem, no margin.
  omega_unit = max R / (u [E_form + E_chol + E_inv + E_inv2])                            reported; the device's is held to 8 x max(restatement's, 1).

SOLVE.  w = the permuted solution of the factored system (K1: P dy), rhs = its right-hand side in long double (K1: P (xi_p + A D xi_d)),
q_i = the entries of row i of A.  The device forms rhs with q_i products fl(fl(D_k xi_d_k) a_ik), q_i additions: (q_i + 3) u (|xi_p| + |A| D |xi_d|)_i.
Forward: y_b = fl(X^_b r_b), r_b = rhs_b - sum L[b, <b] y; backward: x_b = fl(X^_b' z_b).  Write L_bb X^_b = I + E, |E| <= 96 u M16_b M_b
(above; a right residual in both kernels), so that X^_b^-1 = L_bb - E L_bb to first order.  The products round as y_b = X^_b r_b + d,
|d| <= gamma_64 |X_b||r_b|, i.e. r_b = X^_b^-1 (y_b - d), and likewise z_b = X^_b^-T (x_b - d'):
  L_bb y_b - r_b  = E L_bb y_b + L_bb d,        |.| <= (96 M16_b M_b + 64 M_b) |L_bb| |y_b| u,
  L_bb' x_b - z_b = (E L_bb)' x_b + L_bb' d',   |.| <= (96 M16_b M_b |L_bb| + 64 M_b |L_bb|)' |x_b| u
-- expressed through the computed y_b, x_b the backward sweep needs no left residual X^ L - I (bounding it through |z_b| <= |L_bb'||x_b|
would cost two more factors M_b).  With
  L~  = |L| with every diagonal block replaced by M_b |L_bb|          (the plain right residual),
  L~2 = zero but for the diagonal blocks M16_b M_b |L_bb|             (the extra factor of the inverse's residual, both sweeps),
  |rhs - K^ w| <= u [ c_s (L~ (|L'||w|) + |L| (L~' |w|)) + 96 (L~2 (|L'||w|) + |L| (L~2' |w|)) + (factor allowance) |w| + rhs allowance ],   c_s = N + 130
(two sweeps with row sums of length <= N, two products with 64-wide inverses; S between the sweeps is exact).  omega_hard / omega_unit as
above (unit: every coefficient 1).  K1's dx_j = D_j (A_j' dy - xi_d_j) is checked entry by entry against the device's own dy at
(nnz_j + 3) u D_j (|A_j|'|dy| + |xi_d_j|).

ROWS.  R costs a long-double product per row (no BLAS).  N <= 1100: every row.  Above: 96 evenly spaced rows, the last 64, and for the widest
front the two rows on either side of each of its 64-column block boundaries -- never fewer than 160 rows, each against ALL its columns.
The allowances and the solve residual are evaluated for every row at any N.

WHY 8.  omega_hard is loose by about N: a kernel 100 x noisier than it should be (a square root that is not correctly rounded, an accumulation
in the wrong precision) stays under 1 at these sizes.  omega_unit is a maximum of rounding noise over up to N^2 / 2 entries; between two
summation orders of the same algorithm it varies about 3 x (blocked numpy 6.6, LAPACK 19.9 on one input), and the matrix cores' chunks of
four and the split-K part orders are further orders of that kind -- whereas one entry that is 1e-13 relative off gives omega_unit ~ 1e3.

RESTATEMENT.  `restate` is the same algorithm in numpy on a double K: right-looking over the handle's diagonal blocks, explicit inverses,
L_21 = S_21 X' S, block sweeps through the inverses.  It is the guard of the inputs (a GPU test first asserts that the restatement is inside
the bound: otherwise "bad test input") and the yardstick of omega_unit."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, ("tests/backward_error.py needs a long double with a 64-bit significand (x87 extended or wider); "
                                         f"this platform's np.longdouble has eps = {np.finfo(LD).eps}: the residual identities cannot be evaluated here")
U = 2.0 ** -53
C_INV, C_INV2, C_RSQ = 128.0, 96.0, 4.0
ALL_ROWS_UP_TO = 1100


# ---------------------------------------------------------------------------------------------------------------------------------
# the factored matrix of a handle
# ---------------------------------------------------------------------------------------------------------------------------------
def normal_matrix(A, d, dtype):
    """A diag(d) A' as a dense array of `dtype`, summed term by term in that type (no BLAS for long double)."""
    m = A.shape[0]
    d = np.asarray(d).astype(dtype)
    if not sp.issparse(A):
        Ad = np.asarray(A).astype(dtype)
        if dtype is not LD:
            return (Ad * d[None, :]) @ Ad.T
        K = np.zeros((m, m), dtype)                                   # the lower triangle by row blocks, mirrored: half the long-double products
        for r0 in range(0, m, 64):
            r1 = min(r0 + 64, m)
            K[r0:r1, :r1] = (Ad[r0:r1] * d[None, :]) @ Ad[:r1].T
        return np.tril(K) + np.tril(K, -1).T
    K = np.zeros((m, m), dtype)
    A = A.tocsc()
    cnt = np.diff(A.indptr)
    for c in np.unique(cnt[cnt > 0]):
        cols = np.nonzero(cnt == c)[0]
        idx = A.indptr[cols][:, None] + np.arange(c)[None, :]
        r = A.indices[idx]
        v = A.data[idx].astype(dtype)
        vd = v * d[cols][:, None]
        shape = (cols.size, c, c)
        np.add.at(K, (np.broadcast_to(r[:, :, None], shape).ravel(), np.broadcast_to(r[:, None, :], shape).ravel()),
                  (vd[:, :, None] * v[:, None, :]).ravel())
    return K


class System:
    """K^ (long double and double), its absolute terms F, the term counts p, the signs, the right-hand side of one solve with its allowance,
    and the maps between (dx, dy) and the permuted solution -- for one handle and one set of IPM data."""

    def __init__(self, kind, A, perm, data, dense=None):
        th, rp, rd, xp, xd = (np.asarray(v, dtype=np.float64) for v in data)
        m, n = A.shape
        self.kind, self.A, self.m, self.n, self.data = kind, A, m, n, (th, rp, rd, xp, xd)
        self.perm = perm = np.asarray(perm)
        absA = abs(A) if sp.issparse(A) else np.abs(A)
        patA = (absA != 0).astype(np.float64)
        t = th + rp                                                   # one rounding, as on the device
        if kind == "k1":
            self.N = m
            self.D = D = 1.0 / t
            sign = np.ones(m)
            build = lambda dt: normal_matrix(A, D, dt) + np.diag(rd.astype(dt))                      # noqa: E731
            F = normal_matrix(absA, D, np.float64) + np.diag(np.abs(rd))
            P = normal_matrix(patA, np.ones(n), np.float64) + np.eye(m)
            rhs = xp.astype(LD) + self._matvec(A, (D.astype(LD) * xd.astype(LD)))
            q = np.asarray(patA.sum(axis=1)).ravel()
            ra = np.abs(xp) + np.asarray(absA @ (D * np.abs(xd))).ravel()
            self.sparse_cols = np.ones(n, dtype=bool)
        elif kind == "k2":
            self.N = n + m
            self.D = None
            sign = np.concatenate([-np.ones(n), np.ones(m)])
            Ad = A.toarray() if sp.issparse(A) else np.asarray(A)

            def build(dt):
                K = np.zeros((n + m, n + m), dt)
                K[:n, :n] = np.diag(-t.astype(dt)); K[n:, n:] = np.diag(rd.astype(dt))
                K[n:, :n] = Ad.astype(dt); K[:n, n:] = Ad.T.astype(dt)
                return K
            F = np.abs(build(np.float64))
            P = (F != 0).astype(np.float64)
            rhs = np.concatenate([xd, xp]).astype(LD)
            q = np.zeros(n + m); ra = np.zeros(n + m)                 # the right-hand side is a permutation of the caller's: no arithmetic
        else:
            assert kind == "dense_cols"
            dense = np.asarray(dense)
            k = dense.size
            self.N = m + k
            self.dense = dense
            sc = np.ones(n, dtype=bool); sc[dense] = False
            self.sparse_cols = sc
            self.D = D = np.where(sc, 1.0 / t, 0.0)                  # D_s; the dense columns stay out of A D A'
            sign = np.concatenate([np.ones(m), -np.ones(k)])
            Adn = A[:, dense].toarray()

            def build(dt):
                K = np.zeros((m + k, m + k), dt)
                K[:m, :m] = normal_matrix(A, D, dt) + np.diag(rd.astype(dt))
                K[:m, m:] = Adn.astype(dt); K[m:, :m] = Adn.T.astype(dt)
                K[m:, m:] = np.diag(-t[dense].astype(dt))
                return K
            F = np.zeros((m + k, m + k))
            F[:m, :m] = normal_matrix(absA, D, np.float64) + np.diag(np.abs(rd))
            F[:m, m:] = np.abs(Adn); F[m:, :m] = np.abs(Adn).T; F[m:, m:] = np.diag(np.abs(t[dense]))
            P = np.zeros((m + k, m + k))
            P[:m, :m] = normal_matrix(patA[:, :] @ sp.diags(sc.astype(float)), np.ones(n), np.float64) + np.eye(m)
            P[:m, m:] = Adn != 0; P[m:, :m] = (Adn != 0).T; P[m:, m:] = np.eye(k)
            rhs = np.concatenate([xp.astype(LD) + self._matvec(A, D.astype(LD) * xd.astype(LD)), xd[dense].astype(LD)])
            q = np.concatenate([np.asarray((patA @ sp.diags(sc.astype(float))).sum(axis=1)).ravel(), np.zeros(k)])
            ra = np.concatenate([np.abs(xp) + np.asarray(absA @ (D * np.abs(xd))).ravel(), np.zeros(k)])
        ix = np.ix_(perm, perm)
        self.sign = sign[perm]
        self.K = build(LD)[ix]
        self.K64 = build(np.float64)[ix]
        self.F, self.P = F[ix], P[ix]
        self.rhs = rhs[perm]
        self.rhs_hard = ((q + 3 + q / 2048.0) * ra)[perm]
        self.rhs_unit = ra[perm]

    @staticmethod
    def _matvec(A, x):
        """A @ x in long double, entry by entry (scipy has no long double kernels)."""
        if not sp.issparse(A):
            return np.asarray(A).astype(LD) @ x
        C = A.tocoo()
        out = np.zeros(A.shape[0], LD)
        np.add.at(out, C.row, C.data.astype(LD) * x[C.col])
        return out

    def rhs64(self):
        """The right-hand side in double, formed in double (for the restatement)."""
        th, rp, rd, xp, xd = self.data
        if self.kind == "k2":
            return np.concatenate([xd, xp])[self.perm]
        top = xp + np.asarray(self.A @ (self.D * xd)).ravel()
        return (top if self.kind == "k1" else np.concatenate([top, xd[self.dense]]))[self.perm]

    def permuted(self, dx, dy):
        """The permuted solution w of the factored system that (dx, dy) holds."""
        full = dy if self.kind == "k1" else (np.concatenate([dx, dy]) if self.kind == "k2" else np.concatenate([dy, dx[self.dense]]))
        return np.asarray(full, dtype=np.float64)[self.perm]

    def unpermuted(self, w):
        """(dx, dy) of a permuted solution, dx of the eliminated columns formed in double as the device does."""
        th, rp, rd, xp, xd = self.data
        sol = np.zeros(self.N); sol[self.perm] = w
        if self.kind == "k2":
            return sol[: self.n], sol[self.n:]
        dy = sol[: self.m]
        dx = self.D * (np.asarray(self.A.T @ dy).ravel() - xd)
        if self.kind == "dense_cols":
            dx[self.dense] = sol[self.m:]
        return dx, dy


def blocks_of(kkt):
    """(first column, width) of every diagonal block the device inverts, in permuted numbering, ascending."""
    col0, ns = kkt.symbolic("front_col0"), kkt.symbolic("front_ns")
    out = sorted((int(c) + 64 * b, min(64, int(w) - 64 * b)) for c, w in zip(col0, ns) for b in range((int(w) + 63) // 64))
    assert all(a[0] + a[1] == b[0] for a, b in zip(out, out[1:])) and out[0][0] == 0, "the fronts' pivot columns do not tile 0 .. N - 1"
    return out


def rows_to_check(N, kkt):
    """Every row up to ALL_ROWS_UP_TO; above, the deterministic sample of the module docstring."""
    if N <= ALL_ROWS_UP_TO:
        return np.arange(N)
    rows = set(np.linspace(0, N - 1, 96).round().astype(int).tolist()) | set(range(N - 64, N))
    col0, ns = kkt.symbolic("front_col0"), kkt.symbolic("front_ns")
    s = int(np.argmax(ns))
    for b in range(1, (int(ns[s]) + 63) // 64):
        edge = int(col0[s]) + 64 * b
        rows |= {edge - 2, edge - 1, edge, edge + 1}
    rows = np.array(sorted(r for r in rows if 0 <= r < N))
    assert rows.size >= 160, f"the row sample holds {rows.size} rows: fewer than 160"
    return rows


def dense_L_of_emulator(em, N):
    """Dense L (permuted numbering, order N) from the working panels of a tests/emulate.py executor."""
    L = np.zeros((N, N))
    for s in range(len(em.f)):
        if em.local[s]:
            P = em.panel(s); rows = em.rows(s); c0 = int(em.col0[s])
            for c in range(int(em.ns[s])):
                L[rows[c:], c0 + c] = P[c:, c]
    return L


# ---------------------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------------------
def inverse_lower(T):
    """Inverse of a lower triangular block in long double, by forward substitution."""
    w = T.shape[0]
    X = np.zeros((w, w), LD)
    for r in range(w):
        e = np.zeros(w, LD); e[r] = 1
        X[r] = (e - T[r, :r] @ X[:r]) / T[r, r]
    return X


class Allowances:
    """The allowance matrices of a factor L (doubles, lower triangles) and the block data the solve bound needs."""

    def __init__(self, system, L, blocks):
        N = system.N
        assert L.shape == (N, N) and np.isfinite(L).all(), "the factor holds a non-finite entry"
        self.system, self.L, self.blocks = system, L, blocks
        self.absL = absL = np.abs(L)
        self.E_chol = absL @ absL.T
        self.E_inv, self.E_inv2 = np.zeros((N, N)), np.zeros((N, N))
        self.Lt, self.Lt2 = absL.copy(), np.zeros((N, N))
        for c0, w in blocks:
            c1 = c0 + w
            Lbb = np.tril(L[c0:c1, c0:c1])
            X = inverse_lower(Lbb.astype(LD))
            M = np.abs(Lbb) @ np.abs(X).astype(np.float64)
            M16 = np.zeros((w, w))
            for a in range(0, w, 16):
                M16[a:a + 16, a:a + 16] = M[a:a + 16, a:a + 16]      # = |L_ii||X_ii|: the diagonal sub-blocks of a triangular product
            T1 = M @ np.abs(Lbb)                                     # M_b |L_bb|
            T2 = M16 @ T1                                            # M16_b M_b |L_bb|
            self.Lt[c0:c1, c0:c1] = T1
            self.Lt2[c0:c1, c0:c1] = T2
            below = absL[c1:, c0:c1]
            nz = np.nonzero(below.any(axis=1))[0]
            self.E_inv[c1 + nz, c0:c1] = below[nz] @ T1.T            # |L_21| |L_bb'| M_b'
            self.E_inv2[c1 + nz, c0:c1] = below[nz] @ T2.T           # |L_21| |L_bb'| M_b' M16_b'
        ev = N / 2048.0
        self.hard = ((system.P + 3 + system.P / 2048.0) * system.F + (N + 1 + C_RSQ + ev) * self.E_chol
                     + (C_INV + ev) * self.E_inv + (C_INV2 + ev) * self.E_inv2)
        self.unit = system.F + self.E_chol + self.E_inv + self.E_inv2

    def symmetric(self, M):
        T = np.tril(M)
        return T + np.tril(T, -1).T


def _ratio(r, allow):
    """max r / (u allow) and where; an entry with no allowance must be exactly zero."""
    r = np.asarray(r, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(r == 0, 0.0, r / (U * allow))
    k = int(np.argmax(q)) if q.size else 0
    return (float(q[k]) if q.size else 0.0), k


def factor_stats(allow, rows):
    """omega_hard, omega_unit of R = |K^ - L S L'| over `rows` (each against all its columns <= the row), and the worst entry.  The product is
    formed block column by block column on the rows that hold a nonzero there (the zeros of a sparse factor contribute exact zeros)."""
    sysm, L, N = allow.system, allow.L, allow.system.N
    rows = np.asarray(rows)
    pos = np.full(N, -1); pos[rows] = np.arange(rows.size)
    prod = np.zeros((rows.size, N), LD)
    for c0, w in allow.blocks:
        c1 = c0 + w
        rb = c0 + np.nonzero(L[c0:, c0:c1].any(axis=1))[0]
        sel = rb[pos[rb] >= 0]
        if sel.size:
            V = L[sel, c0:c1].astype(LD) * sysm.sign[c0:c1]
            prod[np.ix_(pos[sel], rb)] += V @ L[rb, c0:c1].astype(LD).T            # long double: every (row, column) pair once per block
    lower = np.arange(N)[None, :] <= rows[:, None]
    r = np.where(lower, np.abs(sysm.K[rows] - prod), 0).astype(np.float64)
    h, kh = _ratio(r.ravel(), allow.hard[rows].ravel())
    un, _ = _ratio(r.ravel(), allow.unit[rows].ravel())
    return dict(hard=h, unit=un, at=(int(rows[kh // N]), int(kh % N)))


def solve_stats(allow, w):
    """omega_hard, omega_unit of |rhs - K^ w| (every row)."""
    sysm, N = allow.system, allow.system.N
    w = np.asarray(w, dtype=np.float64)
    assert np.isfinite(w).all(), "the solution holds a non-finite entry"
    r = np.abs(sysm.rhs - sysm.K @ w.astype(LD))
    aw = np.abs(w)
    t = allow.absL.T @ aw
    s1 = allow.Lt @ t + allow.absL @ (allow.Lt.T @ aw)
    s2 = allow.Lt2 @ t + allow.absL @ (allow.Lt2.T @ aw)
    ev = N / 2048.0
    hard = (N + 130 + ev) * s1 + (C_INV2 + ev) * s2 + allow.symmetric(allow.hard) @ aw + sysm.rhs_hard
    unit = s1 + s2 + allow.symmetric(allow.unit) @ aw + sysm.rhs_unit
    h, kh = _ratio(r, hard)
    un, _ = _ratio(r, unit)
    return dict(hard=h, unit=un, at=kh, allowance=hard)


def dx_stats(system, dx, dy):
    """K1 (and the sparse columns of a handle with dense columns): dx_j = D_j (A_j' dy - xi_d_j) against the device's own dy."""
    th, rp, rd, xp, xd = system.data
    A = system.A
    At = A.T.tocsr() if sp.issparse(A) else np.asarray(A).T
    absAt = abs(At) if sp.issparse(At) else np.abs(At)
    nnz = np.asarray((absAt != 0).sum(axis=1)).ravel()
    want = system.D.astype(LD) * (System._matvec(At, np.asarray(dy).astype(LD)) - xd.astype(LD))
    sel = system.sparse_cols
    r = np.abs(np.asarray(dx).astype(LD) - want)[sel]
    base = (system.D * (np.asarray(absAt @ np.abs(dy)).ravel() + np.abs(xd)))[sel]
    h, kh = _ratio(r, (nnz[sel] + 3 + nnz[sel] / 2048.0) * base)
    un, _ = _ratio(r, base)
    return dict(hard=h, unit=un, at=kh)


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
class NotFactorisable(ArithmeticError):
    pass


def restate(system, blocks):
    """The device's algorithm in numpy on the double K^: (L, permuted solution).  Raises NotFactorisable on a pivot of the wrong sign."""
    S, sg, N = np.tril(system.K64), system.sign, system.N
    L = np.zeros((N, N))
    inv = []
    for c0, w in blocks:
        c1 = c0 + w
        B, s = S[c0:c1, c0:c1].copy(), sg[c0:c1]
        for j in range(w):                                            # the signed Cholesky of the diagonal block
            d = B[j, j]
            if not s[j] * d > 0:
                raise NotFactorisable(f"pivot {c0 + j}: {d}")
            B[j, j] = np.sqrt(abs(d))
            B[j + 1:, j] /= s[j] * B[j, j]
            B[j + 1:, j + 1:] -= s[j] * np.tril(np.outer(B[j + 1:, j], B[j + 1:, j]))
        X = sla.solve_triangular(B, np.eye(w), lower=True)           # the explicit inverse, by forward substitution
        inv.append(X)
        L[c0:c1, c0:c1] = B
        nz = c1 + np.nonzero(S[c1:, c0:c1].any(axis=1))[0]           # (the other rows stay exactly zero)
        if nz.size:
            L21 = (S[nz, c0:c1] @ X.T) * s[None, :]
            L[nz, c0:c1] = L21
            S[np.ix_(nz, nz)] -= np.tril((L21 * s[None, :]) @ L21.T)
    x = system.rhs64().copy()
    for (c0, w), X in zip(blocks, inv):                               # forward
        x[c0:c0 + w] = X @ x[c0:c0 + w]
        x[c0 + w:] -= L[c0 + w:, c0:c0 + w] @ x[c0:c0 + w]
    x *= sg
    for (c0, w), X in zip(blocks[::-1], inv[::-1]):                   # backward
        x[c0:c0 + w] = X.T @ (x[c0:c0 + w] - L[c0 + w:, c0:c0 + w].T @ x[c0 + w:])
    return L, x
