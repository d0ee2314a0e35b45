"""Per-call restatement of the interior-point kernels (ipm_shared.hpp, ipm_kernels.hip, ipm_batch_kernels.hip, tlpk_ipm.cpp).  Test
infrastructure in plain numpy: never imported by the product.  This docstring is the specification of what tests/test_ipm_kernels.py asserts.

One restatement, two evaluations.  Every C entry point is restated as "given every vector the call reads, what does it write and return".
For every output the restatement yields
  r   the value in np.longdouble (64-bit significand), from the DOUBLES the device holds: the vectors are read back with tlpk_ipm_get after
      the call; an output that overwrites its own input is evaluated on the state read before the call;
  M   the same expression with every term replaced by its absolute value;
  K   the number of fp64 roundings on the longest path of the device's formula for that output, counted from the kernel source and
      written beside the formula below (a product with a 0 / 1 flag is exact and not counted; FMA contraction only removes roundings).
The rule, derived and not tuned:   |device - r| <= 2 K u M,   u = 2^-53.   The factor 2 covers the second-order terms and the long-double
evaluation itself; there is no other slack.  The tests print and assert   ratio = |device - r| / (K u M) <= 2.   Where K u M = 0 (copies,
zeros, K = 0) the device must hold r exactly.

  Sums over a vector   K = K_entry + depth,  depth = trips + 8 + ceil(blocks / 64) + 6: the per-thread serial trips of the grid-stride loop,
      the 256-wide LDS tree, the finalize lane's serial walk over the blocks l, l + 64, ..., the 64-lane butterfly.  `blocks` is
      ipm_seg_blocks(length the kernel is launched for) = max(1, min(1024, ceil(len / 256))); trips = ceil(len / (256 blocks)) for a column
      loop and ceil(len / (32 blocks)) for the row kernel (8 lanes per row: 32 rows per workgroup and trip).
  Maxima and minima    are selections: the bound is the largest entry bound among the candidates.
  Row dot products     8 lanes, each serial over ceil(len / 8) entries, then 3 shuffle additions: ceil(len / 8) + 3.
  Column dot products  one thread, serial: max(len, 1).   Dense-matrix handles read A'y and A x from GEMV kernels: K = m and K = n (any
      summation order of t terms has at most t roundings on a path).
  Direction recovery   checked as identities on the FINAL direction: dxl = (-xil + dx - dtau lz) lflag, dzl = (xzl - zl dxl) / xl, the
      xu / zu pair likewise.  Mode 2 adds the accepted direction; the value the kernel held in its register is the final one minus the
      accepted one.  That subtraction is exact here but the device's addition was rounded: 2^-53 (|final| + |accepted|) -- both terms are
      in M and the rounding is counted in K.
  dtau, dkappa, h0     the defining equations h0 dtau = xi_g_ + w'dx_s - b'dy_s and tau dkappa = xi_tk - kappa dtau, with dx_s = dx_final -
      dtau hx (- the accepted direction in mode 2); the reconstruction's terms are in M and its roundings in K.
  The KKT solve        (dx_s, dy_s) against the regularised system with theta, regP, regD read back through the codes 33-35 and the
      right-hand side xid, xip: tests/backward_error.py's solve_stats, omega_unit <= 8 max(restatement's, 1).  Its allowances are dense
      N x N matrices: it runs where the factored matrix has at most SOLVE_CHECK_MAX_N rows (every shape but the long LP).  hx, hy and the
      Mehrotra predictor / corrector are the solve's own output.  The homogeneous predictor / corrector are reconstructed as dy_s = dy_final -
      dtau hy; the bound is asserted on them as it stands.  Mode 2: see NOT_MET.  K1: w = P dy; dx = D (A'dy - xi_d) is the solve kernels'
      own step, test_backward_error.py's subject.
  Step to the boundary recomputed in long double from the device's own direction and iterate over the same entries (negative component):
      2 u |r|, i.e. K = 1 and M = |r|; inf when no component is negative.

The float64 stand-in (`StandIn`, `StandInLib`) has the call-and-read-back interface of libtlpk.so: the same formulas in fp64 in the device's
association, sums through the device's reduction tree (`dev_sum`), KKT solves through scipy's sparse LU.  `StandInLib` takes the place of the
ctypes library object, so DeviceHSD / DeviceMPC / BatchedDeviceHSD drive it unchanged and every check runs on a machine without a GPU.
`StandIn.mut` names ONE deliberate defect (MUTATIONS): each must break a bound, or the checker could not fail.

NOT_MET.  One check of the issue cannot be met, for a reason that is not a defect: the KKT check of the solve inside a MODE 2 call
(tlpk_ipm_newton(2), tlpk_mpc_newton(2), tlpk_ipm_batch_newton(2)).  The kernel adds the accepted direction to the solve's solution in place, so
dy_s = dy_final - accepted (- dtau hy) has to be reconstructed, and a centrality corrector is a SMALL correction of the accepted direction: the
rounding of the kernel's addition, u (|dy_final| + |accepted|), which no subtraction can undo, is larger than dy_s's own backward error by the
ratio |accepted| / |dy_s| -- late in a run many orders of magnitude.  omega_unit of solve_stats on the reconstructed solution, against the limit
8 max(restatement's, 1) -- float64 stand-in (whose solves are scipy's sparse LU; the same reconstruction), every mode 2 case above its limit:
    HSD  31x255 it3 1.5e+01, late 1.2e+12 | 32x256 late 1.1e+13 | 33x257 it3 6.9e+01, late 1.8e+10 | rows late 1.6e+08 |
         9x16384 it3 2.2e+03 (limit 31), late 1.3e+15 (65) | 17x16385 start 3.0e+01 (14), it3 3.7e+04 (37), late 1.1e+15 (14)
    MPC  31x255 late 7.3e+08 | 32x256 late 4.9e+11 | 9x16384 it3 1.4e+01 (9.3), late 2.0e+11 (97) | 17x16385 it3 7.2e+01 (19), late 1.6e+13 (18)
(limit 8 where none is given; the other mode 2 cases are below it).  The MI355X (profiles/ipm_kernel_checks.txt, lines "mode 2"): 17 of its 46
mode 2 calls above their limit, the same cases but for 31x255 start (9.7) and rows it3 (23) more and 9x16384 MPC it3 fewer -- e.g. HSD
31x255 it3 1.8e+01, late 1.1e+11; 9x16384 late 1.3e+15 (limit 80); 17x16385 late 7.9e+14 (12); MPC 17x16385 late 1.6e+13 (16).
The tests print this figure for every mode 2 call and do not assert it.  What stays asserted of a mode 2 call: its right-hand sides, the
recovery identities on the final candidate (they hold the accepted direction's addition), dtau, dkappa, the step to the boundary; and the
solve is the same tlpk_solve_device that modes 0 and 1 call, where the bound is asserted.
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "tests/ipm_reference.py needs a long double with a 64-bit significand"
U = 2.0 ** -53
INF = float("inf")
SOLVE_CHECK_MAX_N = 64

NAMES = ["x", "xl", "xu", "zl", "zu", "y", "dx", "dxl", "dxu", "dzl", "dzu", "dy", "cx", "cxl", "cxu", "czl", "czu", "cy",
         "rp", "rl", "ru", "rd", "thl", "thu", "hx", "hy", "hxid", "xil", "xiu", "xzl", "xzu", "xid", "xip", "theta", "regP", "regD"]
ROW_NAMES = frozenset(("y", "dy", "cy", "rp", "hy", "xip", "regD"))
ITER, ACC, CAND = NAMES[0:6], NAMES[6:12], NAMES[12:18]
RHS = ["xil", "xiu", "xzl", "xzu", "xid", "xip"]
# what a call may write; every other readable vector must come back bit-identical
WRITES = {"residuals": ["rp", "rl", "ru", "rd"], "factor": ["thl", "thu", "theta", "regP", "regD"], "hsolve": ["hxid", "hx", "hy"],
          "newton0": RHS + ACC, "newton1": RHS + ACC, "newton2": RHS + CAND, "hsolve_newton": ["hxid", "hx", "hy"] + RHS + ACC,
          "targets": ["xzl", "xzu"], "accept": ACC + CAND, "advance": ITER, "mpc_gap": [], "mpc_targets": ["xzl", "xzu"]}
MUTATIONS = ["rd_signs", "xxu_flag", "last_row", "second_trip", "upper_clamp", "dxl_dtau", "mode2_dzu", "slots", "mpc_alpha", "inactive_xil"]


def seg_blocks(length):
    """ipm_seg_blocks / ipm_blocks: the workgroups launched for a vector of `length`."""
    return int(max(1, min(1024, (length + 255) // 256)))


def depth(length, nb, per=1):
    """Roundings of the reduction of `length` entries by `nb` workgroups: trips + LDS tree + finalize walk + butterfly."""
    trips = max(1, -(-int(length) // (nb * (256 // per))))
    return trips + 8 + -(-nb // 64) + 6


def dev_sum(vals, nb, per=1, first_trip_only=False):
    """The device's order of summation in fp64: grid-stride accumulators, the 256-wide tree, lane l over the blocks l, l + 64, ..., butterfly."""
    vals = np.asarray(vals, dtype=np.float64)
    ent = nb * (256 // per)
    trips = max(1, -(-vals.size // ent))
    buf = np.zeros(trips * ent); buf[:vals.size] = vals
    arr = buf.reshape(trips, ent)
    acc = np.zeros(ent)
    for t in range(1 if first_trip_only else trips):
        acc = acc + arr[t]
    blk = np.zeros((nb, 256)); blk[:, ::per] = acc.reshape(nb, 256 // per)
    s = 128
    while s:
        blk[:, :s] = blk[:, :s] + blk[:, s:2 * s]
        s //= 2
    nl = -(-nb // 64)
    p = np.zeros(nl * 64); p[:nb] = blk[:, 0]
    r = np.zeros(64)
    for row in p.reshape(nl, 64):
        r = r + row
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        r = r + r[lanes ^ off]
    return float(r[0])


class LPData:
    """A standard-form LP as tlpk_ipm_load keeps it: A column- and row-major, b, c, lz = l .* lflag, uz = u .* uflag, the flags as 0 / 1."""

    def __init__(self, A, b, c, l, u, dense=False):
        self.dense = bool(dense)
        self.A = sp.csc_matrix(A).astype(np.float64); self.A.sort_indices()
        self.T = self.A.tocsr(); self.T.sort_indices()
        self.m, self.n = self.A.shape
        self.b, self.c = np.asarray(b, np.float64), np.asarray(c, np.float64)
        self.l, self.u = np.asarray(l, np.float64), np.asarray(u, np.float64)
        self.lf, self.uf = np.isfinite(self.l).astype(np.float64), np.isfinite(self.u).astype(np.float64)
        self.lz, self.uz = np.where(self.lf != 0, self.l, 0.0), np.where(self.uf != 0, self.u, 0.0)
        self.colcnt, self.rowcnt = np.diff(self.A.indptr), np.diff(self.T.indptr)
        self.colof = np.repeat(np.arange(self.n), self.colcnt)            # column of every stored entry, column-major order
        self.rowof = np.repeat(np.arange(self.m), self.rowcnt)            # row of every stored entry, row-major order

    def aty(self, y):
        """A'y in long double: (r, M, K per column)."""
        y = np.asarray(y).astype(LD)
        t = self.A.data.astype(LD) * y[self.A.indices]
        r, M = np.zeros(self.n, LD), np.zeros(self.n, LD)
        np.add.at(r, self.colof, t); np.add.at(M, self.colof, np.abs(t))
        K = np.full(self.n, self.m) if self.dense else np.maximum(self.colcnt, 1)
        return r, M, K

    def ax(self, x):
        x = np.asarray(x).astype(LD)
        t = self.T.data.astype(LD) * x[self.T.indices]
        r, M = np.zeros(self.m, LD), np.zeros(self.m, LD)
        np.add.at(r, self.rowof, t); np.add.at(M, self.rowof, np.abs(t))
        K = np.full(self.m, self.n) if self.dense else -(-self.rowcnt // 8) + 3
        return r, M, K


# ---------------------------------------------------------------------------------------------------------------------------------
# the record of one run of checks
# ---------------------------------------------------------------------------------------------------------------------------------
class Report:
    """Collects ratio = |device - r| / (K u M) per output; `bad` lists the outputs above 2 (or not exact where K u M = 0)."""

    def __init__(self, tag=""):
        self.tag, self.rows, self.bad = tag, [], []

    def _push(self, label, ratio, where=None):
        self.rows.append((label, float(ratio)))
        if not ratio <= 2.0:
            self.bad.append(f"{self.tag} {label}: ratio {float(ratio):.3e}" + ("" if where is None else f" at {where}"))

    def vec(self, label, dev, r, M, K):
        dev = np.atleast_1d(np.asarray(dev, dtype=np.float64)); r = np.atleast_1d(np.asarray(r, dtype=LD))
        bound = np.atleast_1d(np.asarray(K * U * np.asarray(M, dtype=LD), dtype=LD)) * np.ones(dev.shape, LD)
        if dev.size == 0:
            return self._push(label, 0.0)
        same = (dev.astype(LD) == r) | (np.isinf(dev) & np.isinf(r) & (np.sign(dev) == np.sign(r).astype(np.float64)))
        with np.errstate(all="ignore"):
            err = np.where(same, LD(0), np.abs(dev.astype(LD) - r))
            q = np.where(same, LD(0), np.where(bound > 0, err / np.where(bound > 0, bound, 1), LD(INF)))
        q = np.where(np.isnan(q.astype(np.float64)), INF, q.astype(np.float64))
        k = int(np.argmax(q))
        self._push(label, q[k], k)

    def maximum(self, label, dev, r_entries, M_entries, K_entries):
        """A selection: max |r_j| against the largest entry bound."""
        r = np.abs(np.asarray(r_entries, LD)).max(initial=LD(0))
        bound = (np.asarray(K_entries) * U * np.asarray(M_entries, LD)).max(initial=LD(0))
        err = abs(LD(float(dev)) - r)
        self._push(label, 0.0 if err == 0 else (float(err / bound) if bound > 0 else INF))

    def exact(self, label, a, b):
        a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
        ok = a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
        self._push(label + " (bits)", 0.0 if ok else INF, None if ok else int(np.argmax(a.view(np.uint64) != b.view(np.uint64))) if a.shape == b.shape else "shape")

    def unchanged(self, call, pre, post, but=()):
        skip = set(WRITES[call]) | set(but)
        for name in NAMES:
            if name not in skip:
                self.exact(f"{call}: {name} untouched", pre[name], post[name])

    def worst(self):
        return max((r for _, r in self.rows), default=0.0)


def _ld(d, names):
    return [np.asarray(d[k]).astype(LD) for k in names]


def _flagdiv(num, den, flag):
    """num / den where flag != 0, else 0 (long double)."""
    with np.errstate(all="ignore"):
        return np.where(flag != 0, num / np.where(flag != 0, den, 1), LD(0))


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement, call by call.  lp: LPData; pre / post: {name: vector} read before / after the call; rep: Report
# ---------------------------------------------------------------------------------------------------------------------------------
def check_residuals(lp, pre, post, tau, out, rep):
    """tlpk_ipm_residuals (k_ipm_res_cols / k_ipm_res_rows; HSD.jl:77-128, 136-196)."""
    x, xl, xu, zl, zu, y = _ld(post, ITER)
    tau = LD(tau)
    lf, uf, lz, uz, b, c = (v.astype(LD) for v in (lp.lf, lp.uf, lp.lz, lp.uz, lp.b, lp.c))
    aty, Maty, Katy = lp.aty(y)
    ax, Max, Kax = lp.ax(x)
    # rl = (-x + xl + tau lz) lf: fl(-x + xl), fl(tau lz), their sum -- longest path 2
    rl, Mrl = (-x + xl + tau * lz) * lf, (np.abs(x) + np.abs(xl) + np.abs(tau * lz)) * lf
    ru, Mru = (-x - xu + tau * uz) * uf, (np.abs(x) + np.abs(xu) + np.abs(tau * uz)) * uf
    # rd = ((tau c - aty) + zu uf) - zl lf: aty's K, then three additions
    rd, Mrd, Krd = tau * c - aty + zu * uf - zl * lf, np.abs(tau * c) + Maty + np.abs(zu) * uf + np.abs(zl) * lf, Katy + 3
    # rp = tau b - ax: the lane dot product, one subtraction
    rp, Mrp, Krp = tau * b - ax, np.abs(tau * b) + Max, Kax + 1
    rep.vec("rl", post["rl"], rl, Mrl, 2); rep.vec("ru", post["ru"], ru, Mru, 2)
    rep.vec("rd", post["rd"], rd, Mrd, Krd); rep.vec("rp", post["rp"], rp, Mrp, Krp)
    dn, dm = depth(lp.n, seg_blocks(lp.n)), depth(lp.m, seg_blocks(lp.m), per=8)

    def total(label, dev, terms, Kentry, d):
        rep.vec(label, dev, terms.sum(), np.abs(terms).sum(), Kentry + d)
    total("out4 c'x", out[4], c * x, 1, dn)
    total("out5 b'y", out[5], b * y, 1, dm)
    total("out6 lz'zl", out[6], lz * zl, 1, dn)
    total("out7 uz'zu", out[7], uz * zu, 1, dn)
    rep.vec("out8 xl'zl+xu'zu", out[8], (xl * zl + xu * zu).sum(), (np.abs(xl * zl) + np.abs(xu * zu)).sum(), 2 + dn)
    rep.maximum("out0 |rp|", out[0], rp, Mrp, Krp)
    rep.maximum("out1 |rl|", out[1], rl, Mrl, 2)
    rep.maximum("out2 |ru|", out[2], ru, Mru, 2)
    rep.maximum("out3 |rd|", out[3], rd, Mrd, Krd)
    rep.maximum("out9 |Ax|", out[9], ax, Max, Kax)
    rep.maximum("out10 |(x-xl)lf|", out[10], (x - xl) * lf, (np.abs(x) + np.abs(xl)) * lf, 1)
    rep.maximum("out11 |(x+xu)uf|", out[11], (x + xu) * uf, (np.abs(x) + np.abs(xu)) * uf, 1)
    rep.maximum("out12 |A'y+zl-zu|", out[12], aty + zl * lf - zu * uf, Maty + np.abs(zl) * lf + np.abs(zu) * uf, Katy + 2)
    rep.unchanged("residuals", pre, post)


def check_factor(lp, pre, post, regP, regD, rep, active=True):
    """tlpk_ipm_factor's vectors (k_ipm_theta; step.jl:24-31).  A parked LP of a batch: theta = regP = regD = 1, thl / thu stay."""
    if not active:
        for name in ("theta", "regP", "regD"):
            rep.exact("parked " + name, post[name], np.ones_like(post[name]))
        rep.unchanged("factor", pre, post, but=("theta", "regP", "regD"))
        for name in ("thl", "thu"):
            rep.exact("parked: " + name + " untouched", pre[name], post[name])
        return
    xl, xu, zl, zu = _ld(post, ["xl", "xu", "zl", "zu"])
    thl, thu = _flagdiv(zl, xl, lp.lf), _flagdiv(zu, xu, lp.uf)                  # one division each
    rep.vec("thl", post["thl"], thl, np.abs(thl), 1); rep.vec("thu", post["thu"], thu, np.abs(thu), 1)
    rep.vec("theta", post["theta"], thl + thu, np.abs(thl) + np.abs(thu), 2)     # division, then the sum
    rep.exact("regP", post["regP"], np.full(lp.n, float(regP))); rep.exact("regD", post["regD"], np.full(lp.m, float(regD)))
    rep.unchanged("factor", pre, post)


def _h_sum(lp, post):
    """The two sums of k_ipm_hdots and their final addition: (r, M, K)."""
    thl, thu, hx, hy = _ld(post, ["thl", "thu", "hx", "hy"])
    lz, uz, b, c = (v.astype(LD) for v in (lp.lz, lp.uz, lp.b, lp.c))
    # lz (lz tl) + uz (uz tu) - (c + tl lz + tu uz) hx: the last product sits behind three roundings and one subtraction follows: 5
    t = lz * (lz * thl) + uz * (uz * thu) - (c + thl * lz + thu * uz) * hx
    Mt = np.abs(lz * lz * thl) + np.abs(uz * uz * thu) + (np.abs(c) + np.abs(thl * lz) + np.abs(thu * uz)) * np.abs(hx)
    nb = seg_blocks(max(lp.n, lp.m))
    K = max(5 + depth(lp.n, nb), 1 + depth(lp.m, nb)) + 1
    return t.sum() + (b * hy).sum(), Mt.sum() + np.abs(b * hy).sum(), K


def check_hsolve(lp, pre, post, out, rep, call="hsolve"):
    """tlpk_ipm_hsolve (k_ipm_hrhs, k_ipm_hdots; step.jl:56-76).  hx, hy themselves: the KKT check of the test (solve_stats)."""
    thl, thu = _ld(post, ["thl", "thu"])
    lz, uz, c = (v.astype(LD) for v in (lp.lz, lp.uz, lp.c))
    # hxid = (c - thl lz) - thu uz: product, two subtractions: 3
    rep.vec("hxid", post["hxid"], c - thl * lz - thu * uz, np.abs(c) + np.abs(thl * lz) + np.abs(thu * uz), 3)
    r, M, K = _h_sum(lp, post)
    if call == "hsolve":
        rep.vec("out0 h-sum", out[0], r, M, K)
        rep.unchanged("hsolve", pre, post)
    return r, M, K


def step_to_boundary(post, which):
    """min over the entries with a negative component of -v / dv, in long double; (primal, dual)."""
    res = []
    for pairs in ((("xl", which[1]), ("xu", which[2])), (("zl", which[3]), ("zu", which[4]))):
        best = LD(INF)
        for v, dv in pairs:
            a, d = np.asarray(post[v]).astype(LD), np.asarray(post[dv]).astype(LD)
            neg = d < 0
            if neg.any():
                best = min(best, (-a[neg] / d[neg]).min())
        res.append(best)
    return res


def check_newton(lp, pre, post, mode, sc, out, rep, mpc=False, paired=False):
    """tlpk_ipm_newton / tlpk_mpc_newton (k_ipm_newton_pre, _dots, _post; step.jl:198-306).  sc = (tau, kappa, h0, xi_g, xi_tk, eta, gmu, delta);
    MPC: eta = 1, delta = 0, dtau = 0 and out = (primal step, dual step)."""
    tau, kappa, h0, xi_g, xi_tk, eta, gmu, delta = (LD(float(v)) for v in sc)
    lf, uf, lz, uz, b, c = (v.astype(LD) for v in (lp.lf, lp.uf, lp.lz, lp.uz, lp.b, lp.c))
    xl, xu, zl, zu = _ld(post, ["xl", "xu", "zl", "zu"])
    rl, ru, rd, rp, thl, thu, hx, hy = _ld(post, ["rl", "ru", "rd", "rp", "thl", "thu", "hx", "hy"])
    a0 = dict(zip(ITER, _ld(pre, ACC)))                                           # the accepted direction BEFORE the call (mode 1 overwrites it)
    zero_n, zero_m = np.zeros(lp.n, LD), np.zeros(lp.m, LD)
    # ---- right-hand sides (k_ipm_newton_pre)
    if mode == 0:       # copies; xz = -(x z) flag: one product
        want = dict(xil=(rl, 0 * rl, 0), xiu=(ru, 0 * ru, 0), xip=(rp, 0 * rp, 0),
                    xzl=(-(xl * zl) * lf, np.abs(xl * zl) * lf, 1), xzu=(-(xu * zu) * uf, np.abs(xu * zu) * uf, 1))
        xd = rd
    elif mode == 1:     # eta-scaled: one product; xz = ((-x z + gmu) - dx dz) flag: the second product is followed by one subtraction, the first by two
        want = dict(xil=(eta * rl, np.abs(eta * rl), 1), xiu=(eta * ru, np.abs(eta * ru), 1), xip=(eta * rp, np.abs(eta * rp), 1),
                    xzl=((-xl * zl + gmu - a0["xl"] * a0["zl"]) * lf, (np.abs(xl * zl) + abs(gmu) + np.abs(a0["xl"] * a0["zl"])) * lf, 3),
                    xzu=((-xu * zu + gmu - a0["xu"] * a0["zu"]) * uf, (np.abs(xu * zu) + abs(gmu) + np.abs(a0["xu"] * a0["zu"])) * uf, 3))
        xd = eta * rd
    else:               # zeros; the targets minus delta on EVERY entry: one subtraction
        pzl, pzu = _ld(pre, ["xzl", "xzu"])
        want = dict(xil=(zero_n, zero_n, 0), xiu=(zero_n, zero_n, 0), xip=(zero_m, zero_m, 0),
                    xzl=(pzl - delta, np.abs(pzl) + abs(delta), 1), xzu=(pzu - delta, np.abs(pzu) + abs(delta), 1))
        xd = zero_n
    for name, (r, M, K) in want.items():
        rep.vec(f"{name}", post[name], r, M, K)
    xil, xiu, xzl, xzu = _ld(post, ["xil", "xiu", "xzl", "xzu"])                  # what the kernel stored is what it went on with
    # xid = (xd - tl) + tu, tl = (xzl + zl xil) / xl: product, sum, division, two more: 5 (xd's own rounding sits on a shorter path)
    tl, tu = _flagdiv(xzl + zl * xil, xl, lf), _flagdiv(xzu - zu * xiu, xu, uf)
    Mtl, Mtu = _flagdiv(np.abs(xzl) + np.abs(zl * xil), np.abs(xl), lf), _flagdiv(np.abs(xzu) + np.abs(zu * xiu), np.abs(xu), uf)
    rep.vec("xid", post["xid"], xd - tl + tu, np.abs(xd) + Mtl + Mtu, 5)
    # ---- the written direction and the register values behind it
    names = CAND if mode == 2 else ACC
    f = dict(zip(ITER, _ld(post, names)))
    add = mode == 2
    acc = a0 if add else {k: (zero_m if k == "y" else zero_n) for k in ITER}
    dtau = LD(0) if mpc else LD(float(out[0]))
    ka = 2 if add else 0                                                          # mode 2: the kernel's addition of the accepted direction and its rounding undone here
    dxr, Mdxr = f["x"] - acc["x"], np.abs(f["x"]) + np.abs(acc["x"]) * add        # the register dx (after + dtau hx)
    # dxl = ((-xil + dx) - dtau lz) lf: longest path 2 (+ ka)
    rep.vec("dxl", f["xl"], (-xil + dxr - dtau * lz) * lf + acc["xl"], (np.abs(xil) + Mdxr + np.abs(dtau * lz)) * lf + np.abs(acc["xl"]), 2 + ka)
    rep.vec("dxu", f["xu"], (xiu - dxr + dtau * uz) * uf + acc["xu"], (np.abs(xiu) + Mdxr + np.abs(dtau * uz)) * uf + np.abs(acc["xu"]), 2 + ka)
    # dzl = (xzl - zl dxl) / xl with the register dxl: product, subtraction, division: 3 (+ ka)
    dxlr, Mdxlr = f["xl"] - acc["xl"], np.abs(f["xl"]) + np.abs(acc["xl"]) * add
    dxur, Mdxur = f["xu"] - acc["xu"], np.abs(f["xu"]) + np.abs(acc["xu"]) * add
    rep.vec("dzl", f["zl"], _flagdiv(xzl - zl * dxlr, xl, lf) + acc["zl"], _flagdiv(np.abs(xzl) + np.abs(zl) * Mdxlr, np.abs(xl), lf) + np.abs(acc["zl"]), 3 + ka)
    rep.vec("dzu", f["zu"], _flagdiv(xzu - zu * dxur, xu, uf) + acc["zu"], _flagdiv(np.abs(xzu) + np.abs(zu) * Mdxur, np.abs(xu), uf) + np.abs(acc["zu"]), 3 + ka)
    # ---- step to the boundary: 2 u |r|
    ap, ad = step_to_boundary(post, names)
    if mpc:
        rep.vec("out0 primal step", out[0], ap, abs(ap) if np.isfinite(ap) else 0, 1)
        rep.vec("out1 dual step", out[1], ad, abs(ad) if np.isfinite(ad) else 0, 1)
    else:
        a = min(ap, ad)
        rep.vec("out2 step", out[2], a, abs(a) if np.isfinite(a) else 0, 1)
        # ---- dtau, dkappa: the defining equations with the solve's own solution dx_s = register dx - dtau hx
        dxs, Mdxs = dxr - dtau * hx, Mdxr + np.abs(dtau * hx)
        dys, Mdys = f["y"] - acc["y"] - dtau * hy, np.abs(f["y"]) + np.abs(acc["y"]) * add + np.abs(dtau * hy)
        w, Mw = c + thl * lz + thu * uz, np.abs(c) + np.abs(thl * lz) + np.abs(thu * uz)
        ixl, ixu = _flagdiv(xzl, xl, lf), _flagdiv(xzu, xu, uf)
        terms = [-(ixl * lz), ixu * uz, -(thl * xil * lz), -(thu * xiu * uz), w * dxs, -(b * dys)]
        Mterms = [np.abs(ixl * lz), np.abs(ixu * uz), np.abs(thl * xil * lz), np.abs(thu * xiu * uz), Mw * Mdxs, np.abs(b) * Mdys]
        num = xi_g + xi_tk / tau + sum(t.sum() for t in terms)
        Mnum = abs(xi_g) + abs(xi_tk / tau) + sum(t.sum() for t in Mterms)
        nb = seg_blocks(max(lp.n, lp.m))
        d = max(depth(lp.n, nb), depth(lp.m, nb))
        # longest path: w dx_s (w: 3, product: 4; dx_s reconstructed: + 1 + ka / 2) -> sum (depth) -> + q4, - q5, / h0 (3); the path of the first
        # sum: entry 2 -> depth -> six additions and the division (7).  Both are at most depth + 9 + ka.
        rep.vec("out0 dtau", out[0], num / h0, Mnum / abs(h0), d + 9 + ka)
        # dkappa = (xi_tk - kappa dtau) / tau: 3
        rep.vec("out1 dkappa", out[1], (xi_tk - kappa * dtau) / tau, (abs(xi_tk) + abs(kappa * dtau)) / abs(tau), 3)
    if not paired:
        rep.unchanged(f"newton{mode}", pre, post)
    # the solve's own solution (reconstructed where dtau != 0 or the accepted direction was added) and right-hand side, for the KKT check
    return dict(dx=np.asarray(f["x"] - acc["x"] - dtau * hx, np.float64), dy=np.asarray(f["y"] - acc["y"] - dtau * hy, np.float64),
                xip=post["xip"], xid=post["xid"], mode=mode)


def check_hsolve_newton(lp, pre, post, sc, out, rep):
    """tlpk_ipm_hsolve_newton: tlpk_ipm_hsolve + tlpk_ipm_newton(mode 0) with h0 = ((h-sum) + kappa / tau) + regG formed inside (two more roundings)."""
    tau, kappa, regG = (LD(float(v)) for v in sc[:3])
    r, M, K = check_hsolve(lp, pre, post, None, rep, call="hsolve_newton")
    rep.vec("out3 h0", out[3], r + kappa / tau + regG, M + abs(kappa / tau) + abs(regG), K + 2)
    sc2 = np.array(sc, dtype=np.float64); sc2[2] = out[3]
    sol = check_newton(lp, pre, post, 0, sc2, out, rep, paired=True)
    rep.unchanged("hsolve_newton", pre, post)
    return sol


def targets_entries(lp, post, a_p, a_d, mu_l, mu_u):
    """v = ((x + a_p dx)(z + a_d dz)) flag mapped to the box, in long double: (vl, vu, Mvl, Mvu, branch counts).  Product, sum, product: 3;
    the clamp subtracts once more: 4.  The map is continuous, so an entry the device places on the other side of mu_l / mu_u is inside the
    same bound; M takes the larger of |mu_l|, |mu_u| for every bounded entry."""
    a_p, a_d, mu_l, mu_u = (LD(float(v)) for v in (a_p, a_d, mu_l, mu_u))
    res, cnt = [], []
    for v, z, dv, dz, fl in (("xl", "zl", "dxl", "dzl", lp.lf), ("xu", "zu", "dxu", "dzu", lp.uf)):
        x, zz, dx, dzz = _ld(post, [v, z, dv, dz])
        val = (x + a_p * dx) * (zz + a_d * dzz)
        Mv = (np.abs(x) + np.abs(a_p * dx)) * (np.abs(zz) + np.abs(a_d * dzz))
        on = fl != 0
        lo, hi = on & (val < mu_l), on & (val > mu_u)
        r = np.where(lo, mu_l - val, np.where(hi, mu_u - val, LD(0)))
        res += [r, np.where(on, Mv + max(abs(mu_l), abs(mu_u)), LD(0))]
        cnt.append((int(lo.sum()), int((on & ~lo & ~hi).sum()), int(hi.sum())))
    return res[0], res[2], res[1], res[3], cnt


def check_targets(lp, pre, post, a_p, a_d, mu_l, mu_u, out, rep, call="targets"):
    """tlpk_ipm_targets / tlpk_mpc_targets (k_ipm_targets; step.jl:333-364).  Returns the branch counts [(below, inside, above)] x {lower, upper}."""
    vl, vu, Ml, Mu, cnt = targets_entries(lp, post, a_p, a_d, mu_l, mu_u)
    rep.vec("xzl", post["xzl"], vl, Ml, 4); rep.vec("xzu", post["xzu"], vu, Mu, 4)
    if out is not None:
        dn = depth(lp.n, seg_blocks(lp.n))
        rep.vec("out0 sum vl", out[0], vl.sum(), Ml.sum(), 4 + dn); rep.vec("out1 sum vu", out[1], vu.sum(), Mu.sum(), 4 + dn)
    rep.unchanged(call, pre, post)
    return cnt


def check_accept(pre, post, rep, batched=False):
    """tlpk_ipm_accept: the buffers swap roles.  tlpk_ipm_batch_accept: the candidate is COPIED over the accepted direction (and stays)."""
    for a, c in zip(ACC, CAND):
        rep.exact(f"accept: {a} = candidate", post[a], pre[c])
        rep.exact(f"accept: {c}", post[c], pre[c] if batched else pre[a])
    rep.unchanged("accept", pre, post)


def check_advance(lp, pre, post, ap, ad, out, rep):
    """tlpk_ipm_advance / tlpk_mpc_advance (k_ipm_advance; step.jl:139-148): v + alpha dv, a product and a sum: 2."""
    ap, ad = LD(float(ap)), LD(float(ad))
    for v, dv, a in (("x", "dx", ap), ("xl", "dxl", ap), ("xu", "dxu", ap), ("zl", "dzl", ad), ("zu", "dzu", ad), ("y", "dy", ad)):
        p, d = _ld(pre, [v, dv])
        rep.vec(v, post[v], p + a * d, np.abs(p) + np.abs(a * d), 2)
    xl, xu, zl, zu = _ld(post, ["xl", "xu", "zl", "zu"])                          # the new point, as stored
    nb = seg_blocks(max(lp.n, lp.m))
    rep.vec("out0 xl'zl+xu'zu", out[0], (xl * zl + xu * zu).sum(), (np.abs(xl * zl) + np.abs(xu * zu)).sum(), 2 + depth(lp.n, nb))
    rep.unchanged("advance", pre, post)


def check_mpc_gap(lp, pre, post, ap, ad, out, rep):
    """tlpk_mpc_gap (k_mpc_gap): ((xl + ap dxl) lf)(zl + ad dzl) + the xu term: product, sum, product, sum: 4; xl zl + xu zu: 2."""
    ap, ad = LD(float(ap)), LD(float(ad))
    xl, xu, zl, zu, dxl, dxu, dzl, dzu = _ld(post, ["xl", "xu", "zl", "zu", "dxl", "dxu", "dzl", "dzu"])
    lf, uf = lp.lf.astype(LD), lp.uf.astype(LD)
    t = ((xl + ap * dxl) * lf) * (zl + ad * dzl) + ((xu + ap * dxu) * uf) * (zu + ad * dzu)
    M = ((np.abs(xl) + np.abs(ap * dxl)) * lf) * (np.abs(zl) + np.abs(ad * dzl)) + ((np.abs(xu) + np.abs(ap * dxu)) * uf) * (np.abs(zu) + np.abs(ad * dzu))
    dn = depth(lp.n, seg_blocks(lp.n))
    rep.vec("out0 gap after", out[0], t.sum(), M.sum(), 4 + dn)
    rep.vec("out1 gap", out[1], (xl * zl + xu * zu).sum(), (np.abs(xl * zl) + np.abs(xu * zu)).sum(), 2 + dn)
    rep.unchanged("mpc_gap", pre, post)


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 stand-in for the device
# ---------------------------------------------------------------------------------------------------------------------------------
class StandIn:
    """The device vectors of one handle (one LP, or a stack of LPs: row_off / col_off) in numpy, and the kernels on a segment of them."""

    def __init__(self, lp, row_off=None, col_off=None, mut=None):
        self.lp, self.mut = lp, mut
        self.v = {name: np.zeros(lp.m if name in ROW_NAMES else lp.n) for name in NAMES}
        self.row_off = np.array([0, lp.m]) if row_off is None else np.asarray(row_off)
        self.col_off = np.array([0, lp.n]) if col_off is None else np.asarray(col_off)
        self.nlp = len(self.row_off) - 1
        self.batched = row_off is not None
        self.lu = None
        self._blocks = [lp.A[self.seg(k)[1], self.seg(k)[0]].tocsc() for k in range(self.nlp)]
        self.reset()

    # -- helpers
    def seg(self, k):
        return slice(int(self.col_off[k]), int(self.col_off[k + 1])), slice(int(self.row_off[k]), int(self.row_off[k + 1]))

    def _aty(self, cs):
        """Column dot products in the thread's serial order."""
        A, y = self.lp.A, self.v["y"]
        cols = np.arange(cs.start, cs.stop)
        out = np.zeros(cols.size)
        cnt, p0 = self.lp.colcnt[cs], A.indptr[cs.start:cs.stop]
        for t in range(int(cnt.max(initial=0))):
            on = cnt > t
            p = p0[on] + t
            out[on] = out[on] + A.data[p] * y[A.indices[p]]
        return out

    def _ax(self, rs):
        """Row dot products: 8 lanes, each serial over its entries, then the shuffle tree."""
        T, x = self.lp.T, self.v["x"]
        cnt, p0 = self.lp.rowcnt[rs], T.indptr[rs.start:rs.stop]
        if self.mut == "last_row" and cnt.size % 8 == 1:
            cnt = cnt.copy(); cnt[-1] = 0                                         # the lane group with one live row goes missing
        lanes = np.zeros((8, cnt.size))
        for t in range(int(-(-cnt.max(initial=0) // 8))):
            for l in range(8):
                q = 8 * t + l
                on = cnt > q
                if on.any():
                    p = p0[on] + q
                    lanes[l, on] = lanes[l, on] + T.data[p] * x[T.indices[p]]
        a = lanes[0:4] + lanes[4:8]
        a = a[0:2] + a[2:4]
        return a[0] + a[1]

    def _sum(self, vals, nb, per=1):
        return dev_sum(vals, nb, per, first_trip_only=self.mut == "second_trip")

    def reset(self):
        v, lp = self.v, self.lp
        v["x"][:] = 0; v["y"][:] = 0
        v["xl"][:] = lp.lf; v["zl"][:] = lp.lf; v["xu"][:] = lp.uf; v["zu"][:] = lp.uf

    # -- kernels on one segment (cs: columns, rs: rows)
    def res(self, cs, rs, tau):
        v, lp = self.v, self.lp
        x, xl, xu, zl, zu, y = [v[k][cs] for k in ITER[:5]] + [v["y"][rs]]
        lf, uf, lz, uz, c, b = lp.lf[cs], lp.uf[cs], lp.lz[cs], lp.uz[cs], lp.c[cs], lp.b[rs]
        aty = self._aty(cs)
        rl = (-x + xl + tau * lz) * lf; ru = (-x - xu + tau * uz) * uf
        rd = tau * c - aty + zu * uf - zl * lf
        if self.mut == "rd_signs":
            rd = tau * c - aty - zu * uf + zl * lf
        ax = self._ax(rs)
        rp = tau * b - ax
        live = np.ones(rp.size, dtype=bool)
        if self.mut == "last_row" and rp.size % 8 == 1:
            live[-1] = False
        v["rl"][cs], v["ru"][cs], v["rd"][cs] = rl, ru, rd
        v["rp"][rs] = np.where(live, rp, v["rp"][rs])
        n, m = cs.stop - cs.start, rs.stop - rs.start
        nbc, nbr = seg_blocks(n), seg_blocks(m)
        mx = lambda a: float(np.abs(a).max(initial=0.0))                          # noqa: E731
        xxu = (x + xu) if self.mut == "xxu_flag" else (x + xu) * uf
        o = np.zeros(13)
        o[0] = mx(rp[live]); o[1] = mx(rl); o[2] = mx(ru); o[3] = mx(rd)
        o[4] = self._sum(c * x, nbc); o[5] = self._sum(np.where(live, b * y, 0.0), nbr, per=8)
        o[6] = self._sum(lz * zl, nbc); o[7] = self._sum(uz * zu, nbc); o[8] = self._sum(xl * zl + xu * zu, nbc)
        o[9] = mx(ax[live]); o[10] = mx((x - xl) * lf); o[11] = mx(xxu); o[12] = mx(aty + zl * lf - zu * uf)
        if self.mut == "slots":
            o[6], o[7] = o[7], o[6]
        return o

    def theta(self, cs, rs, regP, regD, active=True):
        v, lp = self.v, self.lp
        if not active:
            v["theta"][cs] = 1.0; v["regP"][cs] = 1.0; v["regD"][rs] = 1.0
            return
        with np.errstate(all="ignore"):
            tl = np.where(lp.lf[cs] != 0, v["zl"][cs] / v["xl"][cs], 0.0); tu = np.where(lp.uf[cs] != 0, v["zu"][cs] / v["xu"][cs], 0.0)
        v["thl"][cs], v["thu"][cs], v["theta"][cs] = tl, tu, tl + tu
        v["regP"][cs] = regP; v["regD"][rs] = regD

    def update(self):
        """KKT.update! on the handle's theta / regP / regD (K1: A D A' + Rd) through scipy's sparse LU."""
        v = self.v
        self.D = 1.0 / (v["theta"] + v["regP"])
        self.lu = []
        for k in range(self.nlp):                                 # block by block: an LP's factor does not depend on what else is stacked
            cs, rs = self.seg(k)
            Ak = self._blocks[k]
            self.lu.append(spla.splu((Ak @ sp.diags(self.D[cs]) @ Ak.T + sp.diags(v["regD"][rs])).tocsc()))

    def solve(self, xip, xid):
        dx, dy = np.zeros(self.lp.n), np.zeros(self.lp.m)
        for k in range(self.nlp):
            cs, rs = self.seg(k)
            Ak, D = self._blocks[k], self.D[cs]
            dy[rs] = self.lu[k].solve(xip[rs] + Ak @ (D * xid[cs]))
            dx[cs] = D * (Ak.T @ dy[rs] - xid[cs])
        return dx, dy

    def hrhs(self, cs):
        v, lp = self.v, self.lp
        v["hxid"][cs] = lp.c[cs] - v["thl"][cs] * lp.lz[cs] - v["thu"][cs] * lp.uz[cs]

    def hdots(self, cs, rs):
        v, lp = self.v, self.lp
        lz, uz, tl, tu = lp.lz[cs], lp.uz[cs], v["thl"][cs], v["thu"][cs]
        nb = seg_blocks(max(cs.stop - cs.start, rs.stop - rs.start))
        return (self._sum(lz * (lz * tl) + uz * (uz * tu) - (lp.c[cs] + tl * lz + tu * uz) * v["hx"][cs], nb), self._sum(lp.b[rs] * v["hy"][rs], nb))

    def targets(self, cs, a_p, a_d, mu_l, mu_u):
        v, lp = self.v, self.lp
        out = []
        for x, z, dx, dz, fl, dst in (("xl", "zl", "dxl", "dzl", lp.lf[cs], "xzl"), ("xu", "zu", "dxu", "dzu", lp.uf[cs], "xzu")):
            val = ((v[x][cs] + a_p * v[dx][cs]) * (v[z][cs] + a_d * v[dz][cs])) * fl
            hi = mu_l if self.mut == "upper_clamp" else mu_u
            val = np.where(fl != 0, np.where(val < mu_l, mu_l - val, np.where(val > mu_u, hi - val, 0.0)), val)
            v[dst][cs] = val
            out.append(self._sum(val, seg_blocks(cs.stop - cs.start)))
        return out

    def newton_pre(self, cs, rs, mode, eta, gmu, delta):
        v, lp = self.v, self.lp
        lf, uf, xl, xu, zl, zu = lp.lf[cs], lp.uf[cs], v["xl"][cs], v["xu"][cs], v["zl"][cs], v["zu"][cs]
        if mode == 0:
            xil, xiu, xd = v["rl"][cs].copy(), v["ru"][cs].copy(), v["rd"][cs]
            xzl, xzu = -(xl * zl) * lf, -(xu * zu) * uf
        elif mode == 1:
            xil, xiu, xd = eta * v["rl"][cs], eta * v["ru"][cs], eta * v["rd"][cs]
            xzl = (-xl * zl + gmu - v["dxl"][cs] * v["dzl"][cs]) * lf; xzu = (-xu * zu + gmu - v["dxu"][cs] * v["dzu"][cs]) * uf
        else:
            xil = np.zeros(xl.size); xiu = np.zeros(xl.size); xd = np.zeros(xl.size)
            xzl, xzu = v["xzl"][cs] - delta, v["xzu"][cs] - delta
        v["xil"][cs], v["xiu"][cs], v["xzl"][cs], v["xzu"][cs] = xil, xiu, xzl, xzu
        with np.errstate(all="ignore"):
            tl = np.where(lf != 0, (xzl + zl * xil) / xl, 0.0); tu = np.where(uf != 0, (xzu - zu * xiu) / xu, 0.0)
            ixl = np.where(lf != 0, xzl / xl, 0.0); ixu = np.where(uf != 0, xzu / xu, 0.0)
        v["xid"][cs] = xd - tl + tu
        v["xip"][rs] = v["rp"][rs] if mode == 0 else (eta * v["rp"][rs] if mode == 1 else 0.0)
        nb = seg_blocks(max(cs.stop - cs.start, rs.stop - rs.start))
        return [self._sum(ixl * lp.lz[cs], nb), self._sum(ixu * lp.uz[cs], nb), self._sum((v["thl"][cs] * xil) * lp.lz[cs], nb), self._sum((v["thu"][cs] * xiu) * lp.uz[cs], nb)]

    def newton_dots(self, cs, rs, dst):
        v, lp = self.v, self.lp
        nb = seg_blocks(max(cs.stop - cs.start, rs.stop - rs.start))
        return [self._sum((lp.c[cs] + v["thl"][cs] * lp.lz[cs] + v["thu"][cs] * lp.uz[cs]) * v[dst[0]][cs], nb), self._sum(lp.b[rs] * v[dst[5]][rs], nb)]

    def newton_post(self, cs, rs, dst, add, dtau):
        v, lp = self.v, self.lp
        lf, uf = lp.lf[cs], lp.uf[cs]
        dx = v[dst[0]][cs] + dtau * v["hx"][cs]
        lzt = 0.0 if self.mut == "dxl_dtau" else dtau * lp.lz[cs]
        dxl = (-v["xil"][cs] + dx - lzt) * lf; dxu = (v["xiu"][cs] - dx + dtau * lp.uz[cs]) * uf
        with np.errstate(all="ignore"):
            dzl = np.where(lf != 0, (v["xzl"][cs] - v["zl"][cs] * dxl) / v["xl"][cs], 0.0)
            dzu = np.where(uf != 0, (v["xzu"][cs] - v["zu"][cs] * dxu) / v["xu"][cs], 0.0)
        dy = v[dst[5]][rs] + dtau * v["hy"][rs]
        if add:
            dx = dx + v["dx"][cs]; dxl = dxl + v["dxl"][cs]; dxu = dxu + v["dxu"][cs]; dzl = dzl + v["dzl"][cs]
            if self.mut != "mode2_dzu":
                dzu = dzu + v["dzu"][cs]
            dy = dy + v["dy"][rs]
        for name, val in zip(dst[:5], (dx, dxl, dxu, dzl, dzu)):
            v[name][cs] = val
        v[dst[5]][rs] = dy

        def amin(pairs):
            best = INF
            for a, d in pairs:
                neg = d < 0
                if neg.any():
                    best = min(best, float((-a[neg] / d[neg]).min()))
            return best
        return amin(((v["xl"][cs], dxl), (v["xu"][cs], dxu))), amin(((v["zl"][cs], dzl), (v["zu"][cs], dzu)))

    def advance(self, cs, rs, ap, ad):
        v = self.v
        if self.mut == "mpc_alpha":
            ap = ad
        v["x"][cs] = v["x"][cs] + ap * v["dx"][cs]
        for a, d, al in (("xl", "dxl", ap), ("xu", "dxu", ap), ("zl", "dzl", ad), ("zu", "dzu", ad)):
            v[a][cs] = v[a][cs] + al * v[d][cs]
        v["y"][rs] = v["y"][rs] + ad * v["dy"][rs]
        nb = seg_blocks(max(cs.stop - cs.start, rs.stop - rs.start))
        return self._sum(v["xl"][cs] * v["zl"][cs] + v["xu"][cs] * v["zu"][cs], nb)

    def swap(self):
        for a, c in zip(ACC, CAND):
            self.v[a], self.v[c] = self.v[c], self.v[a]


def _arr(ptr, count, dtype=np.float64):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double if dtype == np.float64 else C.c_uint8)), shape=(int(count),))


def newton_scalars(q, tau, kappa, h0, xi_g, xi_tk):
    """step.jl:232-246 in the association of tlpk_ipm.cpp."""
    xi_g_ = xi_g + xi_tk / tau - q[0] + q[1] - q[2] - q[3]
    with np.errstate(all="ignore"):
        dtau = np.float64(xi_g_ + q[4] - q[5]) / np.float64(h0)
        dkappa = (xi_tk - kappa * dtau) / np.float64(tau)
    return float(dtau), float(dkappa)


class StandInLib:
    """Takes the place of the ctypes library: the entry points of include/tlpk.h that the device-resident loops call, on a StandIn `handle`."""
    OK, BADARG = 0, 2

    # ---- one LP
    def tlpk_ipm_reset(self, h):
        h.reset(); return 0

    def tlpk_ipm_get(self, h, what, host, length):
        if not 0 <= what <= 35:
            return self.BADARG
        src = h.v[NAMES[what]]
        if length != src.size:
            return self.BADARG
        _arr(host, length)[:] = src
        return 0

    def tlpk_ipm_residuals(self, h, tau, out):
        _arr(out, 13)[:] = h.res(*h.seg(0), float(tau)); return 0

    def tlpk_ipm_factor(self, h, regP, regD):
        h.theta(*h.seg(0), float(regP), float(regD)); h.update(); return 0

    def tlpk_ipm_hsolve(self, h, out):
        cs, rs = h.seg(0)
        h.hrhs(cs)
        h.v["hx"][:], h.v["hy"][:] = h.solve(h.lp.b, h.v["hxid"])
        q = h.hdots(cs, rs)
        _arr(out, 1)[0] = q[0] + q[1]
        return 0

    def tlpk_ipm_targets(self, h, a_, mu_l, mu_u, out):
        _arr(out, 2)[:] = h.targets(h.seg(0)[0], a_, a_, mu_l, mu_u); return 0

    def _newton(self, h, mode, tau, kappa, h0, xi_g, xi_tk, eta, gmu, delta, presolved=None):
        cs, rs = h.seg(0)
        dst = CAND if mode == 2 else ACC
        q = presolved if presolved is not None else h.newton_pre(cs, rs, mode, eta, gmu, delta)
        if presolved is None:
            h.v[dst[0]][:], h.v[dst[5]][:] = h.solve(h.v["xip"], h.v["xid"])
        q = q + h.newton_dots(cs, rs, dst)
        dtau, dkappa = newton_scalars(q, tau, kappa, h0, xi_g, xi_tk)
        ap, ad = h.newton_post(cs, rs, dst, mode == 2, dtau)
        return dtau, dkappa, min(ap, ad)

    def tlpk_ipm_newton(self, h, mode, sc, out):
        _arr(out, 3)[:] = self._newton(h, int(mode), *(float(x) for x in _arr(sc, 8))); return 0

    def tlpk_ipm_hsolve_newton(self, h, sc, out):
        cs, rs = h.seg(0)
        tau, kappa, regG, xi_g, xi_tk, eta, gmu, delta = (float(x) for x in _arr(sc, 8))
        h.hrhs(cs)
        q = h.newton_pre(cs, rs, 0, eta, gmu, delta)
        h.v["hx"][:], h.v["hy"][:] = h.solve(h.lp.b, h.v["hxid"])
        h.v["dx"][:], h.v["dy"][:] = h.solve(h.v["xip"], h.v["xid"])
        qh = h.hdots(cs, rs)
        h0 = ((qh[0] + qh[1]) + kappa / tau) + regG
        o = _arr(out, 4)
        o[:3] = self._newton(h, 0, tau, kappa, h0, xi_g, xi_tk, eta, gmu, delta, presolved=q); o[3] = h0
        return 0

    def tlpk_ipm_accept(self, h):
        h.swap(); return 0

    def tlpk_ipm_advance(self, h, alpha, out):
        _arr(out, 1)[0] = h.advance(*h.seg(0), float(alpha), float(alpha)); return 0

    # ---- Mehrotra
    def tlpk_mpc_start(self, h, out):
        v, lp = h.v, h.lp
        v["theta"][:] = 0; v["regP"][:] = 1; v["regD"][:] = 1e-6; v["xid"][:] = 0; v["hx"][:] = 0; v["xip"][:] = 0; v["hy"][:] = 0
        h.update()
        v["dx"][:], v["y"][:] = h.solve(v["xip"], lp.c)
        v["x"][:], v["dy"][:] = h.solve(lp.b, v["xid"])
        on_l, on_u = lp.lf != 0, lp.uf != 0
        q0 = min(0.0, float((v["x"] - lp.lz)[on_l].min(initial=0.0))); q1 = min(0.0, float((lp.uz - v["x"])[on_u].min(initial=0.0)))
        dxs = 1.0 + max(0.0, -1.5 * q0, -1.5 * q1)
        v["xl"][:] = np.where(on_l, (v["x"] - lp.lz) + dxs, 0.0); v["xu"][:] = np.where(on_u, (lp.uz - v["x"]) + dxs, 0.0)
        z = lp.c - h._aty(slice(0, lp.n)); nb = lp.lf + lp.uf
        with np.errstate(all="ignore"):
            v["zl"][:] = np.where(on_l, z / nb, 0.0); v["zu"][:] = np.where(on_u, -z / nb, 0.0)
        dzs = 1.0 + max(0.0, -1.5 * min(0.0, float(v["zl"].min(initial=0.0))), -1.5 * min(0.0, float(v["zu"].min(initial=0.0))))
        v["zl"][:] = np.where(on_l, v["zl"] + dzs, v["zl"]); v["zu"][:] = np.where(on_u, v["zu"] + dzs, v["zu"])
        nbk = seg_blocks(lp.n)
        mu = h._sum(v["xl"] * v["zl"] + v["xu"] * v["zu"], nbk)
        ddx, ddz = mu / (2.0 * h._sum(v["zl"] + v["zu"], nbk)), mu / (2.0 * h._sum(v["xl"] + v["xu"], nbk))
        for a, d, on in (("xl", ddx, on_l), ("zl", ddz, on_l), ("xu", ddx, on_u), ("zu", ddz, on_u)):
            v[a][:] = np.where(on, v[a] + d, v[a])
        _arr(out, 1)[0] = h._sum(v["xl"] * v["zl"] + v["xu"] * v["zu"], nbk)
        return 0

    def tlpk_mpc_newton(self, h, mode, gmu, out):
        cs, rs = h.seg(0)
        dst = CAND if mode == 2 else ACC
        h.newton_pre(cs, rs, int(mode), 1.0, float(gmu), 0.0)
        h.v[dst[0]][:], h.v[dst[5]][:] = h.solve(h.v["xip"], h.v["xid"])
        _arr(out, 2)[:] = h.newton_post(cs, rs, dst, mode == 2, 0.0)
        return 0

    def tlpk_mpc_gap(self, h, ap, ad, out):
        v, lp = h.v, h.lp
        nb = seg_blocks(lp.n)
        s0 = ((v["xl"] + ap * v["dxl"]) * lp.lf) * (v["zl"] + ad * v["dzl"]) + ((v["xu"] + ap * v["dxu"]) * lp.uf) * (v["zu"] + ad * v["dzu"])
        _arr(out, 2)[:] = (h._sum(s0, nb), h._sum(v["xl"] * v["zl"] + v["xu"] * v["zu"], nb))
        return 0

    def tlpk_mpc_targets(self, h, ap_, ad_, tmin, tmax):
        h.targets(h.seg(0)[0], float(ap_), float(ad_), float(tmin), float(tmax)); return 0

    def tlpk_mpc_advance(self, h, ap, ad, out):
        _arr(out, 1)[0] = h.advance(*h.seg(0), float(ap), float(ad)); return 0

    # ---- a stack of LPs: the kernels above per segment with the LP's scalars; an inactive LP is skipped and its outputs are 0
    def tlpk_ipm_batch_residuals(self, h, tau, out):
        tau, o = _arr(tau, h.nlp), _arr(out, 13 * h.nlp)
        for k in range(h.nlp):
            o[13 * k:13 * k + 13] = h.res(*h.seg(k), float(tau[k]))
        return 0

    def tlpk_ipm_batch_factor(self, h, active, regP, regD, fail_lp):
        act, rP, rD = _arr(active, h.nlp, np.uint8), _arr(regP, h.nlp), _arr(regD, h.nlp)
        for k in range(h.nlp):
            h.theta(*h.seg(k), float(rP[k]), float(rD[k]), active=bool(act[k]))
        h.update()
        fail_lp._obj.value = -1
        return 0

    def _solve_into(self, h, act, xip, xid, dstx, dsty):
        """One solve of the stacked system; only the active LPs' segments are written."""
        dx, dy = h.solve(xip, xid)
        for k in range(h.nlp):
            if act[k]:
                cs, rs = h.seg(k)
                h.v[dstx][cs] = dx[cs]; h.v[dsty][rs] = dy[rs]

    def _batch_newton(self, h, mode, act, sc, out, width, paired):
        sc = sc.reshape(h.nlp, 8)
        dst = CAND if mode == 2 else ACC
        q = {}
        for k in range(h.nlp):
            if act[k]:
                cs, rs = h.seg(k)
                if paired:
                    h.hrhs(cs)
                q[k] = h.newton_pre(cs, rs, mode, *(float(x) for x in sc[k, 5:8]))
                if h.mut == "inactive_xil":
                    for j in range(h.nlp):
                        if not act[j]:
                            h.v["xil"][h.seg(j)[0]] += 1.0
        if paired:
            self._solve_into(h, act, h.lp.b, h.v["hxid"], "hx", "hy")
        self._solve_into(h, act, h.v["xip"], h.v["xid"], dst[0], dst[5])
        out[:] = 0.0
        for k in range(h.nlp):
            if not act[k]:
                continue
            cs, rs = h.seg(k)
            tau, kappa, third, xi_g, xi_tk = (float(x) for x in sc[k, :5])
            if paired:
                qh = h.hdots(cs, rs)
                third = ((qh[0] + qh[1]) + kappa / tau) + third
                out[width * k + 3] = third
            dtau, dkappa = newton_scalars(q[k] + h.newton_dots(cs, rs, dst), tau, kappa, third, xi_g, xi_tk)
            ap, ad = h.newton_post(cs, rs, dst, mode == 2, dtau)
            out[width * k:width * k + 3] = (dtau, dkappa, min(ap, ad))
        return 0

    def tlpk_ipm_batch_hsolve_newton(self, h, active, sc, out):
        return self._batch_newton(h, 0, _arr(active, h.nlp, np.uint8), _arr(sc, 8 * h.nlp), _arr(out, 4 * h.nlp), 4, True)

    def tlpk_ipm_batch_newton(self, h, mode, active, sc, out):
        return self._batch_newton(h, int(mode), _arr(active, h.nlp, np.uint8), _arr(sc, 8 * h.nlp), _arr(out, 3 * h.nlp), 3, False)

    def tlpk_ipm_batch_targets(self, h, active, par, out):
        act, par, o = _arr(active, h.nlp, np.uint8), _arr(par, 3 * h.nlp), _arr(out, 2 * h.nlp)
        o[:] = 0.0
        for k in range(h.nlp):
            if act[k]:
                a_, mu_l, mu_u = (float(x) for x in par[3 * k:3 * k + 3])
                o[2 * k:2 * k + 2] = h.targets(h.seg(k)[0], a_, a_, mu_l, mu_u)
        return 0

    def tlpk_ipm_batch_accept(self, h, active):
        act = _arr(active, h.nlp, np.uint8)
        for k in range(h.nlp):
            if act[k]:
                cs, rs = h.seg(k)
                for a, c in zip(ACC, CAND):
                    s = rs if a == "dy" else cs
                    h.v[a][s] = h.v[c][s]
        return 0

    def tlpk_ipm_batch_advance(self, h, active, alpha, out):
        act, al, o = _arr(active, h.nlp, np.uint8), _arr(alpha, h.nlp), _arr(out, h.nlp)
        o[:] = 0.0
        for k in range(h.nlp):
            if act[k]:
                o[k] = h.advance(*h.seg(k), float(al[k]), float(al[k]))
        return 0


def segment_lp(lp, k, row_off, col_off):
    """LP k of a stacked LPData."""
    r0, r1, c0, c1 = int(row_off[k]), int(row_off[k + 1]), int(col_off[k]), int(col_off[k + 1])
    return LPData(lp.A[r0:r1, c0:c1], lp.b[r0:r1], lp.c[c0:c1], lp.l[c0:c1], lp.u[c0:c1])


def segment(vecs, k, row_off, col_off):
    """The part of every readable vector that LP k owns."""
    return {name: (v[int(row_off[k]):int(row_off[k + 1])] if name in ROW_NAMES else v[int(col_off[k]):int(col_off[k + 1])]) for name, v in vecs.items()}


def read_all(L, h, m, n):
    """Every readable vector of a handle through tlpk_ipm_get: {name: vector}."""
    out = {}
    for code, name in enumerate(NAMES):
        v = np.empty(m if name in ROW_NAMES else n)
        rc = L.tlpk_ipm_get(h, code, v.ctypes.data_as(C.POINTER(C.c_double)), v.size)
        assert rc == 0, f"tlpk_ipm_get({code}) returned {rc}"
        out[name] = v
    return out

