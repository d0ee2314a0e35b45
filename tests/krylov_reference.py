"""k-step restatement of the matrix-free family (conjugate gradients on K1, MINRES and TriCG on K2) in long double with a running error bound, and a
float64 model of the device's gather.  Test infrastructure in plain numpy: never imported by the product.  This docstring is the specification of what
tests/test_krylov_steps.py asserts.

WHY.  The gather of krylov_spmv.hpp hands rows and columns to lanes, workgroups and rounds; an index error there yields a slightly different operator
that is still symmetric, and the method converges on it.  A converged solve compared with LAPACK to sqrt(eps) cannot see one dropped entry, and a digest
recorded from the code pins the defect.  After k = 1, 2, 3 iterations from x = 0 nothing has been damped yet: the iterate is a short closed formula in
the operator's output, entry by entry, and a float64 evaluation of it can be bounded rigorously.

THE PAIR (class B).  Every quantity is a pair (v, e): v in np.longdouble (64-bit significand), and e >= 0 with
    |f - v| <= e (1 + small)     for EVERY float64 evaluation f of the same formulas, the additions of a sum taken in any order,
to first order in u = 2^-53.  Inputs are doubles: e = 0.  With fl(x op y) = (x op y)(1 + d), |d| <= u, and inputs a^, b^ within e_a, e_b of a, b:
  sum        a + b:  |fl(a^ + b^) - (a + b)| <= e_a + e_b + u |a + b|
  product    a b:    |a| e_b + |b| e_a + e_a e_b + u |a b|       (e_a e_b is second order, kept: r'r of a residual that has reached zero is nothing else)
  quotient   a / b:  (e_a + |a / b| e_b) / |b| + u |a / b|
  sqrt       sqrt a: e_a / (2 sqrt a) + u sqrt a                       (IEEE: correctly rounded; where e_a > 2^-10 a, the image of [a - e_a, a + e_a])
  hypot      h = hypot(a, b): (|a| e_a + |b| e_b) / h + 2 u h          (one ulp: the library's bound, not a correctly rounded one)
  long sum   s = sum_{q < L} c_q x_q (a row or column of A against a vector, a dot product): every path through ANY summation tree of L terms has at
             most L - 1 additions, and each term is one rounded product:
                 (L + 1) u sum |c_q x_q| + sum (|c_q| e_x + |x_q| e_c + e_c e_x)
             (`extra` adds roundings of the term itself: the Jacobi diagonal's A_ij^2 D_j is two products).  L = 0 gives exactly 0.
             FMA contraction only removes roundings.
Scalars (alpha, beta, the Givens rotation, the 2 x 2 algebra of TriCG) go through the same class.  The derivatives are exact for the operation at hand;
what first order neglects is of relative size e / |v| of the operand that is divided by, and B refuses (BoundError) where that exceeds 2^-10 (the
factor 2 of the rule then has room for a thousand such terms), so that a step beyond the end of the Krylov space (1 x 1 after one step) fails as a bad
input and not as a device failure.

THE RULE.  |device - v| <= 2 e, entry by entry; the factor 2 is tests/ipm_reference.py's: the neglected second-order terms and the long-double evaluation
itself (L 2^-64 against L 2^-53).  Nothing is fitted.  Where e = 0 (x = 0 entries that nothing adds to) the device must hold v exactly.  The bound
grows geometrically with k -- e of one step enters the next one's operator, multiplied by |S| -- so k stays in {1, 2, 3}: k = 1 exposes the right-hand
side, the preconditioner and the scalar p'Sp, k = 2 and 3 the operator's output entry by entry.

THE RESTATEMENTS (cg_steps, minres_steps, tricg_steps) use the formulas of tests/test_krylov.py's cg_restatement, test_krylov_k2.py's
minres_restatement and test_krylov_sqd.py's tricg_restatement, in the device's association (krylov_kernels.hip, krylov_k2_kernels.hip,
krylov_sqd_kernels.hip), generic in the arithmetic: `arith=LongDouble` carries the pairs, `arith=Float64` is plain numpy float64 (the guard of the tests:
the float64 restatement must itself sit inside 2 e).  They run exactly k iterations with no stopping test and return, after each of the k iterations,
what the device returns with itmax = that count: CG dy = x_k and dx = D (A'dy - xi_d); MINRES and TriCG [dx; dy]; resid0 and resid.

THE MODEL (GatherModel) is the unmarked "cpu" driver: the same solve in float64 with every row and column sum formed item by item as walk_short and
walk_long distribute them -- the workgroup counts of krylov_geometry, rounds of parts T / LANES items, the <= CG_LONG test, the long lists strided by
the number of sharing workgroups, lane-strided partial sums, the shuffle trees, the partial sums per workgroup added in slot order.  It does not claim
the device's bits; it reproduces WHICH lane of WHICH workgroup in WHICH round adds WHICH entry, so that a defect can be planted: `mut` names one of
MUTATIONS, and each must break the rule on the case built for it, or the rule could not fail.  A vector the device would leave unwritten keeps its
previous content (zero at create, where the device's is arbitrary)."""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "tests/krylov_reference.py needs a long double with a 64-bit significand"
U = LD(2.0) ** -53
EPS = float(np.finfo(np.float64).eps)
SQRT_EPS = float(np.sqrt(EPS))
FIRST_ORDER = LD(2.0) ** -10

CG_LONG, CG_MAX_SLOTS, CG_MAX_LONG, CG_THREADS, OP_THREADS = 512, 256, 64, 256, 1024          # tlpk_device.hpp, krylov_reduce.hpp, the kernel files
ROW_LANES, COL_LANES = 8, 4

MUTATIONS = ["one_round",        # 1  the second round of a capped short grid is not run
             "long_one_trip",    # 2  the second trip of a long-list workgroup is not run
             "lt_long",          # 3  < CG_LONG instead of <=: an item of exactly 512 entries belongs to neither list
             "short_513",        # 4  an item of 513 entries is walked as short and truncated at 512
             "last_group",       # 5  i < n_items - 1: the last lane group is dropped
             "lane_one_trip",    # 6  the lane loop stops after one trip: entries beyond LANES dropped
             "vec_one_trip",     # 7  the vector kernels' grid-stride loop makes one trip only
             "row_block_offset", # 8  the row half of k_mr_op / k_tc_op reads its block offset without subtracting g_cols
             "long_no_acc",      # 9  a long row's contribution to the kernel's dot product is not added to its slot
             "jacobi_no_long"]   # 10 the Jacobi gather drops the long rows


class BoundError(ArithmeticError):
    """the first-order analysis does not hold at this operand: a bad input (the Krylov space is exhausted), not a device failure"""


# ---------------------------------------------------------------------------------------------------------------------------------
# the two arithmetics
# ---------------------------------------------------------------------------------------------------------------------------------
def _segsum(vals, indptr):
    out = np.zeros(len(indptr) - 1, dtype=vals.dtype)
    ne = np.flatnonzero(np.diff(indptr) > 0)
    if ne.size:
        out[ne] = np.add.reduceat(vals, indptr[ne])
    return out


class B:
    """(v, e): a long-double value and the first-order bound of the module's docstring"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=LD)
        self.e = np.zeros(self.v.shape, dtype=LD) if e is None else np.asarray(e, dtype=LD)

    @staticmethod
    def of(x):
        return x if isinstance(x, B) else B(x)

    def _resolved(self, what):
        if np.any(self.e > FIRST_ORDER * np.abs(self.v)):
            raise BoundError(f"{what}: an operand's bound exceeds 2^-10 of its value")

    def __neg__(self):
        return B(-self.v, self.e)

    def __add__(self, o):
        o = B.of(o); v = self.v + o.v
        return B(v, self.e + o.e + U * np.abs(v))

    def __sub__(self, o):
        o = B.of(o); v = self.v - o.v
        return B(v, self.e + o.e + U * np.abs(v))

    def __mul__(self, o):
        o = B.of(o); v = self.v * o.v
        return B(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e + U * np.abs(v))

    def __truediv__(self, o):
        o = B.of(o); o._resolved("quotient")
        v = self.v / o.v
        return B(v, (self.e + np.abs(v) * o.e) / np.abs(o.v) + U * np.abs(v))

    def __getitem__(self, k):
        return B(self.v[k], self.e[k])

    def sqrt(self):
        if np.any(self.v < 0):
            raise BoundError("sqrt of a negative value")
        r = np.sqrt(self.v)
        if np.all(self.e <= FIRST_ORDER * self.v):
            return B(r, self.e / (2 * r) + U * r)
        hi = np.sqrt(self.v + self.e)          # not resolved (a residual that has reached zero): the interval itself
        return B(r, np.maximum(hi - r, r - np.sqrt(np.maximum(self.v - self.e, 0))) + U * hi)


class LongDouble:
    """the arithmetic of the pairs"""
    name = "long double"

    @staticmethod
    def exact(x):
        return B(np.asarray(x, dtype=np.float64))

    @staticmethod
    def zeros(k):
        return B(np.zeros(k, dtype=LD))

    @staticmethod
    def concat(a, b):
        return B(np.concatenate([a.v, b.v]), np.concatenate([a.e, b.e]))

    @staticmethod
    def hypot(a, b):
        h = np.hypot(a.v, b.v)
        if not h > 0:
            raise BoundError("hypot of two zeros")
        return B(h, (np.abs(a.v) * a.e + np.abs(b.v) * b.e) / h + 2 * U * h)

    @staticmethod
    def dot(a, b):
        t = a.v * b.v
        return B(t.sum(), (t.size + 1) * U * np.abs(t).sum() + (np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e).sum())

    @staticmethod
    def gather(coef, idx, indptr, x, extra=0):
        """s_i = sum_{q in item i} coef_q x[idx_q]; coef: doubles (exact) or their squares"""
        c = np.asarray(coef, dtype=LD)
        t = c * x.v[idx]
        L = np.diff(indptr).astype(LD)
        return B(_segsum(t, indptr), (L + 1 + extra) * U * _segsum(np.abs(t), indptr) + _segsum(np.abs(c) * x.e[idx], indptr))

    @staticmethod
    def positive(a):
        return bool(np.all(a.v - a.e > 0))


class Float64:
    """plain numpy float64: the restatement as tests/test_krylov*.py state it"""
    name = "float64"
    exact = staticmethod(lambda x: np.asarray(x, dtype=np.float64))
    zeros = staticmethod(lambda k: np.zeros(k))
    concat = staticmethod(lambda a, b: np.concatenate([a, b]))
    hypot = staticmethod(np.hypot)
    dot = staticmethod(lambda a, b: np.dot(a, b))
    positive = staticmethod(lambda a: bool(np.all(a > 0)))

    @staticmethod
    def gather(coef, idx, indptr, x, extra=0):
        return _segsum(np.asarray(coef, dtype=np.float64) * x[idx], indptr)


def _sqrt(a):
    return a.sqrt() if isinstance(a, B) else np.sqrt(a)


def values(q):
    """the float64 view of a quantity of either arithmetic"""
    return np.asarray(q.v if isinstance(q, B) else q, dtype=np.float64)


class _Mat:
    """A as the handle keeps it: its CSC copy and its row-wise copy, the gathers of both"""

    def __init__(self, A, ar):
        self.C = sp.csc_matrix(A).astype(np.float64); self.C.sort_indices()
        self.T = self.C.tocsr(); self.T.sort_indices()
        self.m, self.n = self.C.shape
        self.ar = ar

    def rows(self, x, sq=False):          # A x (sq: (A .* A) x, two products per term)
        T = self.T
        return self.ar.gather(T.data.astype(LD) ** 2 if sq else T.data, T.indices, T.indptr, x, extra=1 if sq else 0)

    def cols(self, y):                    # A'y
        C = self.C
        return self.ar.gather(C.data, C.indices, C.indptr, y)


# ---------------------------------------------------------------------------------------------------------------------------------
# the three restatements: exactly k iterations, no stopping test; a list of k snapshots
# ---------------------------------------------------------------------------------------------------------------------------------
def cg_steps(A, th, rp, rd, xp, xd, precond=None, k=1, arith=LongDouble):
    """conjugate gradients on (A D A' + Rd) dy = xi_p + A D xi_d from x = 0 -> [dict(dx, dy, resid0, resid)] after iterations 1 .. k"""
    ar = arith; M = _Mat(A, ar); ex = ar.exact
    one = ex(1.0); rd_, xd_ = ex(rd), ex(xd)
    D = one / (ex(th) + ex(rp))
    b = ex(xp) + M.rows(D * xd_)
    Minv = one / (M.rows(D, sq=True) + rd_) if precond == "jacobi" else None
    x = ar.zeros(M.m); r = b
    z = Minv * r if Minv is not None else r
    p = z
    gamma = ar.dot(r, z)
    resid0 = _sqrt(gamma)
    out = []
    for it in range(k):
        q = M.rows(D * M.cols(p)) + rd_ * p
        alpha = gamma / ar.dot(p, q)
        x = x + alpha * p
        r = r - alpha * q
        z = Minv * r if Minv is not None else r
        g1 = ar.dot(r, z)
        out.append(dict(dy=x, dx=D * (M.cols(x) - xd_), resid0=resid0, resid=_sqrt(g1)))
        if it + 1 < k:
            p = z + (g1 / gamma) * p
        gamma = g1
    return out


def exit_gather(A, th, rp, xd, dy, arith=LongDouble):
    """dx = D (A'dy - xi_d) from the doubles dy: CG's exit on its own, with the bound of one gather"""
    ar = arith; M = _Mat(A, ar); ex = ar.exact
    return (ex(1.0) / (ex(th) + ex(rp))) * (M.cols(ex(dy)) - ex(xd))


def minres_steps(A, th, rp, rd, xp, xd, precond=None, k=1, arith=LongDouble):
    """MINRES on [-E A'; A Rd] [dx; dy] = [xi_d; xi_p] -> [dict(dx, dy, resid0, resid)] after iterations 1 .. k"""
    ar = arith; M = _Mat(A, ar); ex = ar.exact
    n = M.n; N = M.n + M.m
    one = ex(1.0); rd_ = ex(rd)
    E = ex(th) + ex(rp)
    if not ar.positive(E):
        raise BoundError("E = theta^-1 + Rp must be positive here (the branch E_j = 0 of the Jacobi kernel is not restated)")
    Minv = ar.concat(one / E, one / (M.rows(one / E, sq=True) + rd_)) if precond == "jacobi" else None
    b = ar.concat(ex(xd), ex(xp))
    z = Minv * b if Minv is not None else b
    beta = _sqrt(ar.dot(b, z))
    resid0 = phibar = beta
    oldb = None
    dbar = eps = sn = ex(0.0); cs = ex(-1.0)
    r1 = None; r2 = b
    x = ar.zeros(N); w1 = ar.zeros(N); w2 = ar.zeros(N)
    out = []
    for it in range(k):
        v = z / beta
        u = ar.concat(M.cols(v[n:]) - E * v[:n], M.rows(v[:n]) + rd_ * v[n:])
        if it:
            u = u - (beta / oldb) * r1
        alpha = ar.dot(v, u)
        rn = u - (alpha / beta) * r2
        zn = Minv * rn if Minv is not None else rn
        betan = _sqrt(ar.dot(rn, zn))
        oldeps = eps
        delta = cs * dbar + sn * alpha
        gbar = sn * dbar - cs * alpha
        gamma = ar.hypot(gbar, betan)
        if not values(gamma) > EPS:
            raise BoundError("gamma <= eps: the clamp of the rotation is not restated")
        eps = sn * betan; dbar = -(cs * betan)          # (both from the PREVIOUS rotation)
        cs = gbar / gamma; sn = betan / gamma
        phi = cs * phibar; phibar = sn * phibar
        wn = (v - oldeps * w1 - delta * w2) / gamma
        x = x + phi * wn
        w1, w2 = w2, wn
        r1, r2 = r2, rn
        z = zn; oldb = beta; beta = betan
        out.append(dict(dx=x[:n], dy=x[n:], resid0=resid0, resid=phibar))
    return out


def tricg_steps(A, th, rp, rd, xp, xd, precond=None, k=1, arith=LongDouble):
    """TriCG on [Rd A; A' -E] [dy; dx] = [xi_p; xi_d], vectors ordered [n-part; m-part] -> [dict(dx, dy, resid0, resid)] after iterations 1 .. k"""
    assert precond is None
    ar = arith; M = _Mat(A, ar); ex = ar.exact
    n, m = M.n, M.m
    one = ex(1.0)
    W = ar.concat(ex(th) + ex(rp), ex(rd))
    if not ar.positive(W):
        raise BoundError("W = [theta^-1 + Rp; Rd] must be positive")
    Winv = one / W

    def norms(t):
        s = t * Winv
        return _sqrt(ar.dot(s[:n], t[:n])) if n else ex(0.0), _sqrt(ar.dot(s[n:], t[n:])) if m else ex(0.0)

    def scaled(t, gamma, beta):
        s = Winv * t
        return ar.concat(s[:n] / gamma, s[n:] / beta)

    t = ar.concat(ex(xd), ex(xp))
    gamma, beta = norms(t)
    w = ar.zeros(n + m)
    x = ar.zeros(n + m); g0 = ar.zeros(n + m); g1 = ar.zeros(n + m)
    resid0 = ar.hypot(beta, gamma)
    i00 = i01 = i11 = pi0 = pi1 = None
    zn, zm = ar.zeros(n), ar.zeros(m)
    out = []
    for it in range(k):
        wo, w = w, scaled(t, gamma, beta)          # (the device forms it at the end of the step before; the last step's is never read)
        u, v = w[:n], w[n:]
        tr = M.rows(u) - gamma * (W[n:] * wo[n:])
        t = ar.concat(M.cols(v) - beta * (W[:n] * wo[:n]), tr)
        alpha = ar.dot(v, tr)
        t = t - alpha * (W * w)
        if it == 0:
            l00 = l01 = l10 = l11 = ex(0.0)
            d00 = one; d01 = alpha; d11 = -one; r0 = beta; r1 = gamma
        else:
            l00 = beta * i01; l01 = beta * i11; l10 = gamma * i00; l11 = gamma * i01
            d00 = one - l01 * beta; d01 = alpha - l00 * gamma; d11 = -one - l10 * gamma
            r0 = -(beta * pi1); r1 = -(gamma * pi0)
        det = d00 * d11 - d01 * d01
        i00 = d11 / det; i01 = -(d01 / det); i11 = d00 / det
        pi0 = i00 * r0 + i01 * r1; pi1 = i01 * r0 + i11 * r1
        gamma_n, beta_n = norms(t)
        c0 = ar.concat(zn, v) - (g0 * l00 + g1 * l01)
        c1 = ar.concat(u, zm) - (g0 * l10 + g1 * l11)
        g0, g1 = c0, c1
        x = x + (c0 * pi0 + c1 * pi1)
        beta, gamma = beta_n, gamma_n
        out.append(dict(dx=x[:n], dy=x[n:], resid0=resid0, resid=ar.hypot(beta_n * pi1, gamma_n * pi0)))
    return out


STEPS = {"cg": cg_steps, "minres": minres_steps, "tricg": tricg_steps}


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 model of the device's gather
# ---------------------------------------------------------------------------------------------------------------------------------
def _tree(v):
    """lane 0 of a shuffle-down tree over the last axis (a power of two)"""
    v = np.array(v, dtype=np.float64)
    off = v.shape[-1] // 2
    while off:
        v[..., :off] = v[..., :off] + v[..., off:2 * off]
        off //= 2
    return v[..., 0]


def block_sum(acc):
    """cg_block_sum: acc[workgroup, thread] -> one sum per workgroup: the 64-lane tree, then the waves in wave order"""
    g, T = acc.shape
    waves = _tree(acc.reshape(g, T // 64, 64))
    s = np.zeros(g)
    for w in range(T // 64):
        s = s + waves[:, w]
    return s


def sum_slots(slots):
    """cg_sum_slots: in slot order"""
    s = 0.0
    for v in np.asarray(slots, dtype=np.float64).tolist():
        s += v
    return s


def lane_sums(term, q0, q1, lanes, one_trip=False):
    """per item: `lanes` lane-strided serial partial sums of term[q0:q1], then the tree"""
    q0 = np.asarray(q0, dtype=np.int64); q1 = np.asarray(q1, dtype=np.int64)
    s = np.zeros((q0.size, lanes))
    if q0.size == 0:
        return s[:, 0]
    trips = int(-(-int((q1 - q0).max(initial=0)) // lanes))
    lane = np.arange(lanes)
    for t in range(min(trips, 1) if one_trip else trips):
        q = q0[:, None] + lane + t * lanes
        ok = q < q1[:, None]
        s = s + np.where(ok, term[np.where(ok, q, 0)], 0.0)          # (adding 0.0 leaves a sum as it is)
    return _tree(s)


def geometry(rowlen, collen, cg, mut=None):
    """krylov_geometry"""
    m, n = len(rowlen), len(collen)
    lim = CG_LONG + 1 if mut == "short_513" else CG_LONG
    g = dict(long_rows=np.flatnonzero(rowlen > lim), long_cols=np.flatnonzero(collen > lim))
    g["g_cols"] = min((n * COL_LANES + OP_THREADS - 1) // OP_THREADS, CG_MAX_SLOTS)
    g["g_rows"] = max(1 if cg else 0, min((m * ROW_LANES + OP_THREADS - 1) // OP_THREADS, CG_MAX_SLOTS))
    g["g_lcols"] = min(len(g["long_cols"]), CG_MAX_LONG)
    g["g_lrows"] = min(len(g["long_rows"]), CG_MAX_LONG)
    g["g_vec"] = max(1, min(((m if cg else n + m) + CG_THREADS - 1) // CG_THREADS, CG_MAX_SLOTS))
    return g


class GatherModel:
    """One handle: create (the geometry), update, solve -- the launches of tlpk_api.cpp's krylov_update and krylov_solve with itmax = k and the default
    tolerances.  solve() -> dx, dy; `stats` holds krylov_iters, krylov_resid0, krylov_resid."""

    def __init__(self, A, method, precond=None, itmax=1, mut=None):
        assert mut is None or mut in MUTATIONS
        self.C = sp.csc_matrix(A).astype(np.float64); self.C.sort_indices()
        self.T = self.C.tocsr(); self.T.sort_indices()
        self.m, self.n = self.C.shape
        self.method, self.jacobi, self.itmax, self.mut = method, precond == "jacobi", int(itmax), mut
        self.geo = geometry(np.diff(self.T.indptr), np.diff(self.C.indptr), method == "cg", mut)
        self.stats = {}

    # -- krylov_spmv.hpp --------------------------------------------------------------------------------------------------------
    def walk_short(self, term, ptr, n_items, T, lanes, parts, done, part0=0):
        """the workgroups part0 .. part0 + parts - 1 of a grid that walks with `parts`; done(items, sums) stores and returns what lane 0 adds to its
        thread's accumulator (or None) -> acc[workgroup, thread]"""
        mut = self.mut
        per = parts * T // lanes
        acc = np.zeros(parts * T)
        for rnd, base in enumerate(range(0, n_items, per)):
            if mut == "one_round" and rnd:
                break
            i = base + part0 * T // lanes + np.arange(per, dtype=np.int64)
            i = i[i < (n_items - 1 if mut == "last_group" else n_items)]
            q0, q1 = ptr[i], ptr[i + 1]
            if mut == "lt_long":
                mine = q1 - q0 < CG_LONG
            elif mut == "short_513":
                mine = q1 - q0 <= CG_LONG + 1
                q1 = np.minimum(q1, q0 + CG_LONG)
            else:
                mine = q1 - q0 <= CG_LONG
            i, q0, q1 = i[mine], q0[mine], q1[mine]
            c = done(i, lane_sums(term, q0, q1, lanes, one_trip=mut == "lane_one_trip"))
            if c is not None:
                acc[(i - base - part0 * T // lanes) * lanes] += c          # lane 0 of the item's group; one item per thread and round
        return acc.reshape(parts, T)

    def walk_long(self, term, ptr, lst, g, stride, T, done):
        """g workgroups; workgroup w takes lst[w], lst[w + stride], ... -> what each one's first thread has accumulated"""
        acc = np.zeros(g)
        for w in range(g):
            for trip, k in enumerate(range(w, len(lst), stride)):
                if self.mut == "long_one_trip" and trip:
                    break
                i = int(lst[k])
                v = term[ptr[i]:ptr[i + 1]]
                buf = np.zeros(-(-v.size // T) * T); buf[:v.size] = v
                th = np.zeros(T)
                for row in buf.reshape(-1, T):
                    th = th + row
                c = done(np.array([i]), block_sum(th[None, :]))
                if c is not None and self.mut != "long_no_acc":
                    acc[w] += c[0]
        return acc

    def own_grid(self, term, ptr, n_items, lanes, lst, done, jacobi=False):
        """k_cg_jacobi, k_mr_jacobi, k_cg_cols: ceil(n_items lanes / 256) workgroups of 256 threads (one round) and a workgroup per long item"""
        self.walk_short(term, ptr, n_items, CG_THREADS, lanes, max(1, -(-n_items * lanes // CG_THREADS)), done)
        if not (jacobi and self.mut == "jacobi_no_long"):
            self.walk_long(term, ptr, lst, len(lst), max(1, len(lst)), CG_THREADS, done)

    def op_grid(self, col_term, col_done, row_term, row_done):
        """k_mr_op, k_tc_op: g_cols + g_rows + g_lcols + g_lrows workgroups of 1024 threads -> the sum of the slots, in slot order"""
        geo, C, T = self.geo, self.C, self.T
        gc, gr = geo["g_cols"], geo["g_rows"]
        slots = [block_sum(self.walk_short(col_term, C.indptr, self.n, OP_THREADS, COL_LANES, gc, col_done)),
                 block_sum(self.walk_short(row_term, T.indptr, self.m, OP_THREADS, ROW_LANES, gr, row_done, part0=gc if self.mut == "row_block_offset" else 0)),
                 self.walk_long(col_term, C.indptr, geo["long_cols"], geo["g_lcols"], geo["g_lcols"], OP_THREADS, col_done),
                 self.walk_long(row_term, T.indptr, geo["long_rows"], geo["g_lrows"], geo["g_lrows"], OP_THREADS, row_done)]
        return sum_slots(np.concatenate(slots))

    # -- the vector kernels -----------------------------------------------------------------------------------------------------
    def covered(self, N):
        """the entries a vector kernel reaches"""
        return min(N, self.geo["g_vec"] * CG_THREADS) if self.mut == "vec_one_trip" else N

    def vec_sum(self, c):
        """the grid-stride accumulators, cg_block_sum, the slots in slot order; c: the addends of the entries reached"""
        g = self.geo["g_vec"]
        per = g * CG_THREADS
        trips = max(1, -(-c.size // per))
        buf = np.zeros(trips * per); buf[:c.size] = c
        acc = np.zeros(per)
        for t in range(trips):
            acc = acc + buf[t * per:(t + 1) * per]
        return sum_slots(block_sum(acc.reshape(g, CG_THREADS)))

    # -- update -----------------------------------------------------------------------------------------------------------------
    def _jacobi_done(self, i, s):
        M = s + self.rd[i]
        self.Minv[self.joff + i] = np.where(M == 0.0, 1.0, 1.0 / np.where(M == 0.0, 1.0, M))

    def update(self, th, rp, rd):
        T = self.T
        self.rd = np.asarray(rd, dtype=np.float64)
        self.E = np.asarray(th, dtype=np.float64) + np.asarray(rp, dtype=np.float64)
        self.D = 1.0 / self.E
        self.Minv = None
        if self.method == "tricg":
            self.W = np.concatenate([self.E, self.rd]); self.Winv = 1.0 / self.W
        elif self.jacobi and self.method == "cg":
            self.Minv = np.zeros(self.m); self.joff = 0
            self.own_grid(T.data * T.data * self.D[T.indices], T.indptr, self.m, ROW_LANES, self.geo["long_rows"], self._jacobi_done, jacobi=True)
        elif self.jacobi:
            E = self.E
            self.Minv = np.zeros(self.n + self.m); self.joff = self.n
            self.Minv[:self.n] = np.where(E == 0.0, 1.0, 1.0 / np.where(E == 0.0, 1.0, E))
            e = E[T.indices]
            self.own_grid(np.where(e > 0.0, T.data * T.data / np.where(e > 0.0, e, 1.0), 0.0), T.indptr, self.m, ROW_LANES, self.geo["long_rows"], self._jacobi_done, jacobi=True)

    # -- solve ------------------------------------------------------------------------------------------------------------------
    def solve(self, xp, xd):
        xp = np.asarray(xp, dtype=np.float64); xd = np.asarray(xd, dtype=np.float64)
        x = {"cg": self._cg, "minres": self._minres, "tricg": self._tricg}[self.method](xp, xd)
        if self.method != "cg":
            return x[:self.n].copy(), x[self.n:].copy()
        C = self.C                                              # k_dx: one thread per column, serial
        return self.D * (lane_sums(C.data * x[C.indices], C.indptr[:-1], C.indptr[1:], 1) - xd), x

    def _cg(self, xp, xd):
        geo, C, T, m, n, D, rd, Minv = self.geo, self.C, self.T, self.m, self.n, self.D, self.rd, self.Minv
        w = D * xd                                              # k_rhs_scale, k_rhs: 8 lanes per row of any length
        b = xp + lane_sums(T.data * w[T.indices], T.indptr[:-1], T.indptr[1:], ROW_LANES)
        cov = self.covered(m)
        tol_of = lambda rho0: SQRT_EPS + SQRT_EPS * rho0
        x = np.zeros(m); p = np.zeros(m); r = b.copy(); t = np.zeros(n); q = np.zeros(m)
        z = Minv[:cov] * r[:cov] if Minv is not None else r[:cov]
        p[:cov] = z
        gamma = self.vec_sum(r[:cov] * z)
        rho0 = rho = float(np.sqrt(gamma))
        tol = tol_of(rho0)
        it = 0
        while rho > tol and it < self.itmax:
            def col_done(j, s):
                t[j] = D[j] * s
            self.own_grid(C.data * p[C.indices], C.indptr, n, COL_LANES, geo["long_cols"], col_done)

            def row_done(i, s):
                q[i] = s + rd[i] * p[i]
                return p[i] * q[i]
            term = T.data * t[T.indices]
            slots = [block_sum(self.walk_short(term, T.indptr, m, OP_THREADS, ROW_LANES, geo["g_rows"], row_done)),
                     self.walk_long(term, T.indptr, geo["long_rows"], geo["g_lrows"], max(1, geo["g_lrows"]), OP_THREADS, row_done)]
            alpha = gamma / sum_slots(np.concatenate(slots))
            x[:cov] += alpha * p[:cov]
            r[:cov] = r[:cov] - alpha * q[:cov]
            z = Minv[:cov] * r[:cov] if Minv is not None else r[:cov]
            g1 = self.vec_sum(r[:cov] * z)
            rho = float(np.sqrt(g1))
            it += 1
            if rho > tol and it < self.itmax:
                p[:cov] = z + (g1 / gamma) * p[:cov]
            gamma = g1
        self.stats = dict(krylov_iters=it, krylov_resid0=rho0, krylov_resid=rho)
        return x

    def _minres(self, xp, xd):
        C, T, m, n, E, rd, Minv = self.C, self.T, self.m, self.n, self.E, self.rd, self.Minv
        N = n + m
        cov = self.covered(N)
        b = np.concatenate([xd, xp])
        r = [np.zeros(N), np.zeros(N)]
        zz = [np.zeros(N), np.zeros(N)] if Minv is not None else r
        r[0][:cov] = b[:cov]
        if Minv is not None:
            zz[0][:cov] = Minv[:cov] * b[:cov]
        beta = float(np.sqrt(self.vec_sum(b[:cov] * zz[0][:cov])))
        rho0 = phibar = beta
        tol = SQRT_EPS + SQRT_EPS * beta
        oldb = 0.0; dbar = 0.0; eps = 0.0; cs = -1.0; sn = 0.0
        x = np.zeros(N); w = [np.zeros(N), np.zeros(N)]; u = np.zeros(N)
        it = 0
        while phibar > tol and it < self.itmax:
            par = it & 1
            z, r1 = zz[par], r[par ^ 1]
            z1, z2 = z[:n], z[n:]
            c1 = 0.0 if it == 0 else beta / oldb

            def col_done(j, s):
                vj = z1[j] / beta
                uj = s - E[j] * vj
                if it:
                    uj = uj - c1 * r1[j]
                u[j] = uj
                return vj * uj

            def row_done(i, s):
                vi = z2[i] / beta
                ui = s + rd[i] * vi
                if it:
                    ui = ui - c1 * r1[n + i]
                u[n + i] = ui
                return vi * ui
            alpha = self.op_grid(C.data * (z2[C.indices] / beta), col_done, T.data * (z1[T.indices] / beta), row_done)
            c2 = alpha / beta
            rn = u[:cov] - c2 * r[par][:cov]
            r[par ^ 1][:cov] = rn
            if Minv is not None:
                zz[par ^ 1][:cov] = Minv[:cov] * rn
            g = self.vec_sum(rn * zz[par ^ 1][:cov])
            betan = float(np.sqrt(g))
            oldeps = eps; delta = cs * dbar + sn * alpha; gbar = sn * dbar - cs * alpha
            gamma = max(float(np.hypot(gbar, betan)), EPS)
            eps = sn * betan; dbar = -cs * betan
            cs = gbar / gamma; sn = betan / gamma
            phi = cs * phibar; phibar = sn * phibar
            wn = (z[:cov] / beta - oldeps * w[par][:cov] - delta * w[par ^ 1][:cov]) / gamma
            w[par][:cov] = wn
            x[:cov] += phi * wn
            oldb = beta; beta = betan
            it += 1
        self.stats = dict(krylov_iters=it, krylov_resid0=rho0, krylov_resid=phibar)
        return x

    def _tricg(self, xp, xd):
        C, T, m, n, W, Winv = self.C, self.T, self.m, self.n, self.W, self.Winv
        N = n + m
        cov = self.covered(N)
        t = np.zeros(N); t[:cov] = np.concatenate([xd, xp])[:cov]
        first = np.arange(cov) < n

        def norms():
            s = t[:cov] * Winv[:cov] * t[:cov]
            return float(np.sqrt(self.vec_sum(np.where(first, s, 0.0)))), float(np.sqrt(self.vec_sum(np.where(first, 0.0, s))))

        def scaled(gamma, beta):
            norm = np.where(first, gamma, beta)
            return np.where(norm > 0.0, Winv[:cov] * t[:cov] / np.where(norm > 0.0, norm, 1.0), 0.0)
        gamma, beta = norms()
        w = [np.zeros(N), np.zeros(N)]
        w[0][:cov] = scaled(gamma, beta)
        x = np.zeros(N); g0 = np.zeros(N); g1 = np.zeros(N)
        rho0 = rho = float(np.hypot(beta, gamma))
        tol = SQRT_EPS + SQRT_EPS * rho0
        i00 = i01 = i11 = pi0 = pi1 = 0.0
        it = 0
        while rho > tol and it < self.itmax:
            par = it & 1
            wc, wo = w[par], w[par ^ 1]
            u, v = wc[:n], wc[n:]

            def col_done(j, s):
                t[j] = s - beta * (W[j] * wo[j])

            def row_done(i, s):
                qi = s - gamma * (W[n + i] * wo[n + i])
                t[n + i] = qi
                return v[i] * qi
            alpha = self.op_grid(C.data * v[C.indices], col_done, T.data * u[T.indices], row_done)
            t[:cov] = t[:cov] - alpha * (W[:cov] * wc[:cov])
            gamma_n, beta_n = norms()
            if it == 0:
                l00 = l01 = l10 = l11 = 0.0
                d00, d01, d11, r0, r1 = 1.0, alpha, -1.0, beta, gamma
            else:
                l00 = beta * i01; l01 = beta * i11; l10 = gamma * i00; l11 = gamma * i01
                d00 = 1.0 - l01 * beta; d01 = alpha - l00 * gamma; d11 = -1.0 - l10 * gamma
                r0 = -beta * pi1; r1 = -gamma * pi0
            det = d00 * d11 - d01 * d01
            i00 = d11 / det; i01 = -d01 / det; i11 = d00 / det
            pi0 = i00 * r0 + i01 * r1; pi1 = i01 * r0 + i11 * r1
            wi, a, b = wc[:cov], g0[:cov], g1[:cov]
            c0 = np.where(first, 0.0, wi) - (a * l00 + b * l01)
            c1 = np.where(first, wi, 0.0) - (a * l10 + b * l11)
            g0[:cov] = c0; g1[:cov] = c1
            x[:cov] += c0 * pi0 + c1 * pi1
            wo[:cov] = scaled(gamma_n, beta_n)
            beta, gamma = beta_n, gamma_n
            rho = float(np.hypot(beta_n * pi1, gamma_n * pi0))
            it += 1
        self.stats = dict(krylov_iters=it, krylov_resid0=rho0, krylov_resid=rho)
        return x
