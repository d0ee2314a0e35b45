"""Test infrastructure for the refinement on demand (tlpk_polish_device): the same loop -- residuals of the augmented system, one more solve with
them as right-hand side, candidate, guard -- in plain numpy on a callable solver, and the residuals and rounding allowances in long double.

    r1 = xi_p - A dx - Rd dy        r2 = xi_d + (theta + Rp) dx - A' dy

The guard is that of csrc/kernels.hip: k_refine_decide: a step is kept only if |r1|inf shrinks and |r2|inf <= 16 x its value at entry; after the first
rejected step the remaining ones change nothing."""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
U = float(np.finfo(np.float64).eps) / 2            # unit roundoff of the kernels' arithmetic


def _coo(A):
    C = sp.coo_matrix(A)
    return C.row, C.col, C.data.astype(LD), C.shape


def residuals_ld(A, th, rp, rd, xp, xd, dx, dy):
    """(r1, r2) evaluated in long double from float64 inputs."""
    row, col, val, (m, n) = _coo(A)
    dxl, dyl = np.asarray(dx, dtype=LD), np.asarray(dy, dtype=LD)
    ax = np.zeros(m, dtype=LD); np.add.at(ax, row, val * dxl[col])
    aty = np.zeros(n, dtype=LD); np.add.at(aty, col, val * dyl[row])
    r1 = np.asarray(xp, dtype=LD) - ax - np.asarray(rd, dtype=LD) * dyl
    r2 = np.asarray(xd, dtype=LD) + (np.asarray(th, dtype=LD) + np.asarray(rp, dtype=LD)) * dxl - aty
    return r1, r2


def norms_ld(A, th, rp, rd, xp, xd, dx, dy):
    r1, r2 = residuals_ld(A, th, rp, rd, xp, xd, dx, dy)
    return float(np.abs(r1).max(initial=0.0)), float(np.abs(r2).max(initial=0.0))


def allowances(A, th, rp, rd, xp, xd, dx, dy):
    """Rounding bounds of the residual kernel's own sums, as one number per norm: max_i (q_i + 3) u (|xi| + |A||x| + diag |x|)_i with q_i the stored
    entries of the row (r1) or column (r2): q_i products and additions of the sum, then the diagonal product and two more additions.  A float64 max-norm
    lies within this of the long-double one (the maximum of perturbed entries moves by at most the largest perturbation)."""
    row, col, val, (m, n) = _coo(A)
    a = np.abs(val); ax = np.abs(np.asarray(dx, dtype=LD)); ay = np.abs(np.asarray(dy, dtype=LD))
    s1 = np.zeros(m, dtype=LD); np.add.at(s1, row, a * ax[col])
    s2 = np.zeros(n, dtype=LD); np.add.at(s2, col, a * ay[row])
    q1 = np.bincount(row, minlength=m); q2 = np.bincount(col, minlength=n)
    e = np.abs(np.asarray(th, dtype=LD) + np.asarray(rp, dtype=LD))
    t1 = (q1 + 3) * U * (np.abs(np.asarray(xp, dtype=LD)) + s1 + np.abs(np.asarray(rd, dtype=LD)) * ay)
    t2 = (q2 + 3) * U * (np.abs(np.asarray(xd, dtype=LD)) + s2 + e * ax)
    return float(t1.max(initial=0.0)), float(t2.max(initial=0.0))


def _resid64(A, AT, th, rp, rd, xp, xd, dx, dy):
    return xp - A @ dx - rd * dy, xd + (th + rp) * dx - AT @ dy


def polish_reference(solve, A, th, rp, rd, xp, xd, dx, dy, steps):
    """The loop of tlpk_polish_device on `solve(xi_p, xi_d) -> (dx, dy)`, float64.  Returns (dx, dy, report); report: accepted, rejected and the four
    norms (r1_in, r2_in, r1, r2) as the library reports them."""
    A = sp.csr_matrix(A); AT = sp.csr_matrix(A.T)
    nrm = lambda v: float(np.abs(v).max(initial=0.0))            # noqa: E731
    dx, dy = np.array(dx, dtype=np.float64), np.array(dy, dtype=np.float64)
    r1, r2 = _resid64(A, AT, th, rp, rd, xp, xd, dx, dy)
    cur1 = in1 = nrm(r1); ref2 = kept2 = nrm(r2)
    accepted = rejected = 0
    for _ in range(steps):
        if rejected:
            break
        cx, cy = solve(r1, r2)
        cx, cy = dx + cx, dy + cy
        c1, c2 = _resid64(A, AT, th, rp, rd, xp, xd, cx, cy)
        n1, n2 = nrm(c1), nrm(c2)
        if n1 < cur1 and n2 <= 16.0 * ref2:
            dx, dy, r1, r2, cur1, kept2 = cx, cy, c1, c2, n1, n2
            accepted += 1
        else:
            rejected += 1
    return dx, dy, {"accepted": accepted, "rejected": rejected, "r1_in": in1, "r2_in": ref2, "r1": cur1, "r2": kept2}
