// krylov_kernels.hip -- matrix-free K1: preconditioned conjugate gradients on S dy = b, S = A D A' + Rd (tlpk_options.krylov; DESIGN.md
// section 1b'''').  S is never formed: one product with S is a pass over the CSC copy of A (t = D .* A'p, by columns) and a pass over
// its row-wise copy (q = A t + Rd .* p, by rows).
//
// One iteration = four launches and no host involvement:
//   k_cg_cols   t = D .* (A' p)
//   k_cg_rows   q = A t + Rd .* p, partial sums of p'q          -> one slot per workgroup
//   k_cg_step   alpha = gamma / p'q;  x += alpha p;  r -= alpha q;  partial sums of r'z, z = M^-1 r     -> one slot per workgroup
//   k_cg_dir    gamma' = r'z;  stopping rule;  beta = gamma' / gamma;  p = z + beta p;  counter, outcome
// Scalars live in CgScalars (tlpk_device.hpp).  A workgroup reduces its partial sum with a fixed shuffle tree and writes it to its slot; every
// workgroup of the consuming kernel adds the slots in slot order.  No atomics: two solves of the same data are bit-identical.  Every kernel reads
// the outcome word first and returns when it is set: iterations enqueued past the end of a solve cost a launch each and change nothing.
// No kernel waits for another one: nothing here can hang.
//
// Rows and columns of an LP hold a handful of entries: 8 lanes per row, 4 per column.  A row or column with more than CG_LONG entries (a linking
// row, a dense column) is listed at create and gets a whole workgroup in the same launch (the blocks behind those of the short ones).
// The gather itself is krylov_spmv.hpp's: a kernel here supplies the addend of an entry and what one lane does with a finished sum.
//
// NR = 2 carries a pair of right-hand sides through the same four launches (krylov_reduce.hpp): sc[0], sc[1], every vector and slot array twice, A, D, Rd
// and M^-1 once.  Each right-hand side is worked on while ITS outcome word says so.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "krylov_reduce.hpp"
#include "krylov_spmv.hpp"
#include "tlpk_device.hpp"

namespace tlpk {

namespace {

constexpr int CG_ROW_THREADS = 1024;    // k_cg_rows: its workgroups are capped at CG_MAX_SLOTS (one partial sum each), so each is as large as it can be

constexpr int CG_SLOTS_LDS = CG_MAX_SLOTS + CG_MAX_LONG;
// M_i = sum_j A_ij^2 D_j + Rd_i, stored inverted.  Blocks [0, gs): 8 lanes per row; blocks behind: one long row each.
__global__ __launch_bounds__(CG_THREADS) void k_cg_jacobi(i64 m, const i64 *__restrict__ Tp, const i32 *__restrict__ Tj, const double *__restrict__ Tx,
                                                          const double *__restrict__ D, const double *__restrict__ regD, double *__restrict__ Minv,
                                                          unsigned gs, const i32 *__restrict__ long_rows) {
    __shared__ double sh[CG_THREADS / 64];
    const auto term = [&](i64 q) { return Tx[q] * Tx[q] * D[Tj[q]]; };
    const auto done = [&](i64 i, double s) { Minv[i] = cg_minv(s + regD[i]); };
    const unsigned n_long = gridDim.x - gs;
    if (blockIdx.x < gs) walk_short<CG_THREADS, 8>(m, Tp, blockIdx.x, gs, term, done);
    else walk_long<CG_THREADS>(long_rows, n_long, blockIdx.x - gs, n_long, Tp, sh, term, done);
}

__device__ __forceinline__ bool cg_running(long long word) { return word == CG_RUNNING; }

// x = 0, p = z = M^-1 r, partial sums of r'z
template <int NR>
__global__ __launch_bounds__(CG_THREADS) void k_cg_init(i64 m, Rc<NR> rr, const double *__restrict__ Minv, Rv<NR> xx, Rv<NR> pp, Rv<NR> slots_v) {
    __shared__ double sh[CG_THREADS / 64];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const double *__restrict__ rv_ = rr.p[r];
        double *__restrict__ x = xx.p[r], *__restrict__ p = pp.p[r];
        double acc = 0.0;
        for (i64 i = (i64)blockIdx.x * CG_THREADS + threadIdx.x; i < m; i += (i64)gridDim.x * CG_THREADS) {
            const double ri = rv_[i], z = Minv ? Minv[i] * ri : ri;
            x[i] = 0.0; p[i] = z;
            acc += ri * z;
        }
        acc = cg_block_sum(acc, sh);
        if (threadIdx.x == 0) slots_v.p[r][blockIdx.x] = acc;
    }
}
// one workgroup (thread r writes the block of right-hand side r): gamma at x = 0, the tolerance of this solve, the outcome word
template <int NR>
__global__ __launch_bounds__(CG_THREADS) void k_cg_init_scalars(CgScalars *__restrict__ scs, Rc<NR> slots_v, int ns, double atol, double rtol, long long itmax) {
    __shared__ double shs[NR * CG_SLOTS_LDS];
    bool on[NR];
    double gs[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) on[r] = true;
    cg_sum_slots<NR, CG_SLOTS_LDS>(slots_v, ns, shs, on, gs);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if (threadIdx.x != r) continue;
        CgScalars *sc = scs + r;
        const double g0 = gs[r];
        const double rho0 = sqrt(g0), tol = atol + rtol * rho0;
        sc->gamma[0] = g0; sc->gamma[1] = g0;
        sc->tol = tol; sc->resid0 = rho0; sc->resid = rho0; sc->pq = 0.0;
        sc->iters = 0; sc->itmax = itmax;
        sc->outcome = !(g0 >= 0.0 && isfinite(g0)) ? CG_BREAKDOWN : (rho0 <= tol ? CG_SOLVED : (itmax <= 0 ? CG_ITMAX : CG_RUNNING));
    }
}

// t = D .* (A' p).  Blocks [0, gs): 4 lanes per column; blocks behind: one long column each.
template <int NR>
__global__ __launch_bounds__(CG_THREADS) void k_cg_cols(const CgScalars *__restrict__ sc, i64 n, const i64 *__restrict__ Ap, const i32 *__restrict__ Ai,
                                                        const double *__restrict__ Ax, const double *__restrict__ D, Rc<NR> p, Rv<NR> t, unsigned gs,
                                                        const i32 *__restrict__ long_cols) {
    __shared__ double sh[CG_THREADS / 64];
    bool on[NR];
    if (!krylov_running<NR>(sc, on)) return;
    const auto entry = [&](i64 q) { return SpEntry{Ax[q], Ai[q]}; };
    const auto term = [&](const SpEntry &e, int r) { return e.a * p.p[r][e.i]; };
    const auto done = [&](i64 j, double s, int r) { t.p[r][j] = D[j] * s; };
    const unsigned n_long = gridDim.x - gs;
    if (blockIdx.x < gs) walk_short<CG_THREADS, 4, NR>(n, Ap, blockIdx.x, gs, on, entry, term, done);
    else walk_long<CG_THREADS, NR>(long_cols, n_long, blockIdx.x - gs, n_long, Ap, sh, on, entry, term, done);
}

// q = A t + Rd .* p and the partial sums of p'q.  Blocks [0, gs): 8 lanes per row, rows handed out round by round (every wave makes the same number
// of rounds); blocks [gs, gs + gl): the long rows, a workgroup per row.  Slot = block index.
template <int NR>
__global__ __launch_bounds__(CG_ROW_THREADS) void k_cg_rows(const CgScalars *__restrict__ sc, i64 m, const i64 *__restrict__ Tp, const i32 *__restrict__ Tj,
                                                        const double *__restrict__ Tx, Rc<NR> t, const double *__restrict__ regD, Rc<NR> p, Rv<NR> qv,
                                                        Rv<NR> slots_r, unsigned gs, unsigned gl, const i32 *__restrict__ long_rows, i64 n_long) {
    __shared__ double sh[CG_ROW_THREADS / 64];
    bool on[NR];
    if (!krylov_running<NR>(sc, on)) return;
    double acc[NR];      // this workgroup's part of p'q: spread over the lanes of the short rows, on the first thread of the long ones
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = 0.0;
    const auto entry = [&](i64 q) { return SpEntry{Tx[q], Tj[q]}; };
    const auto term = [&](const SpEntry &e, int r) { return e.a * t.p[r][e.i]; };
    const auto done = [&](i64 i, double s, int r) { const double pi = p.p[r][i], qi = s + regD[i] * pi; qv.p[r][i] = qi; acc[r] += pi * qi; };
    if (blockIdx.x >= gs) {          // (the long rows first and on a path of their own: testing the short ones first measured 0.5 us per iteration slower)
        walk_long<CG_ROW_THREADS, NR>(long_rows, n_long, blockIdx.x - gs, gl, Tp, sh, on, entry, term, done);
#pragma unroll
        for (int r = 0; r < NR; ++r) if (on[r] && threadIdx.x == 0) slots_r.p[r][blockIdx.x] = acc[r];
        return;
    }
    walk_short<CG_ROW_THREADS, 8, NR>(m, Tp, blockIdx.x, gs, on, entry, term, done);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if (!on[r]) continue;
        acc[r] = cg_block_sum<CG_ROW_THREADS>(acc[r], sh);
        if (threadIdx.x == 0) slots_r.p[r][blockIdx.x] = acc[r];
    }
}

// alpha = gamma / p'q;  x += alpha p;  r -= alpha q;  partial sums of r'z.  p'q <= 0 or a scalar that is not finite: the solve ends as not solved
// (every workgroup sees the same sum and leaves that right-hand side; the first one records it).
template <int NR>
__global__ __launch_bounds__(CG_THREADS) void k_cg_step(CgScalars *__restrict__ sc, int par, i64 m, Rv<NR> xx, Rv<NR> rr, Rc<NR> pp, Rc<NR> qq,
                                                        const double *__restrict__ Minv, Rc<NR> slots_r, int ns_r, Rv<NR> slots_v) {
    __shared__ double sh[CG_THREADS / 64];
    __shared__ double shs[NR * CG_SLOTS_LDS];
    bool on[NR];
    if (!krylov_live<NR>(sc, on, cg_running)) return;
    double pqs[NR];
    cg_sum_slots<NR, CG_SLOTS_LDS>(slots_r, ns_r, shs, on, pqs);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if (!on[r]) continue;
        const double pq = pqs[r];
        const double alpha = sc[r].gamma[par] / pq;
        if (!(pq > 0.0) || !isfinite(pq) || !isfinite(alpha)) {
            if (blockIdx.x == 0 && threadIdx.x == 0) { sc[r].pq = pq; sc[r].outcome = CG_BREAKDOWN; }
            if (NR == 1) return;
            on[r] = false;
            continue;
        }
        double *__restrict__ x = xx.p[r], *__restrict__ rv_ = rr.p[r];
        const double *__restrict__ p = pp.p[r], *__restrict__ qv = qq.p[r];
        double acc = 0.0;
        for (i64 i = (i64)blockIdx.x * CG_THREADS + threadIdx.x; i < m; i += (i64)gridDim.x * CG_THREADS) {
            x[i] += alpha * p[i];
            const double ri = rv_[i] - alpha * qv[i];
            rv_[i] = ri;
            acc += ri * (Minv ? Minv[i] * ri : ri);
        }
        acc = cg_block_sum(acc, sh);
        if (threadIdx.x == 0) slots_v.p[r][blockIdx.x] = acc;
        if (blockIdx.x == 0 && threadIdx.x == 0) sc[r].pq = pq;
    }
}

// gamma' = r'z;  solved when sqrt(gamma') <= tol, tired when k + 1 = itmax;  otherwise p = z + (gamma' / gamma) p.  The first workgroup's first thread
// writes the scalars of the next iteration (the other parity of gamma: the workgroups still running read this iteration's).
template <int NR>
__global__ __launch_bounds__(CG_THREADS) void k_cg_dir(CgScalars *__restrict__ sc, int par, long long k, i64 m, Rc<NR> rr, const double *__restrict__ Minv,
                                                       Rv<NR> pp, Rc<NR> slots_v, int ns_v) {
    __shared__ double shs[NR * CG_SLOTS_LDS];
    bool on[NR];
    if (!krylov_live<NR>(sc, on, cg_running)) return;
    double g1s[NR];
    cg_sum_slots<NR, CG_SLOTS_LDS>(slots_v, ns_v, shs, on, g1s);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if (!on[r]) continue;
        const double g1 = g1s[r];
        const double g0 = sc[r].gamma[par];
        const double rho = sqrt(g1), beta = g1 / g0;
        const long long itmax = sc[r].itmax;
        const bool broken = !(g1 >= 0.0) || !isfinite(g1);
        const bool solved = !broken && rho <= sc[r].tol;
        const bool go_on = !broken && !solved && k + 1 < itmax && isfinite(beta);
        const double *__restrict__ rv_ = rr.p[r];
        double *__restrict__ p = pp.p[r];
        if (go_on)
            for (i64 i = (i64)blockIdx.x * CG_THREADS + threadIdx.x; i < m; i += (i64)gridDim.x * CG_THREADS) {
                const double ri = rv_[i];
                p[i] = (Minv ? Minv[i] * ri : ri) + beta * p[i];
            }
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            sc[r].gamma[par ^ 1] = g1;
            sc[r].resid = rho;
            sc[r].iters = k + 1;
            if (!go_on) sc[r].outcome = solved ? CG_SOLVED : ((broken || !isfinite(beta)) ? CG_BREAKDOWN : CG_ITMAX);
        }
    }
}

// the launches of an init / an iteration for NR right-hand sides: number 0 on c's vectors and the first half of xw, number 1 on c2's and the second half;
// the scalar blocks are sc[0 .. NR)
template <int NR>
void cg_init(hipStream_t st, const DevArrays &a, const CgArrays &c, const CgArrays &c2, CgScalars *sc, double atol, double rtol, i64 itmax) {
    double *const r2 = a.ctx.xw + a.ctx.xw2;
    if (a.m > 0)
        hipLaunchKernelGGL(k_cg_init<NR>, dim3((unsigned)c.geo.g_vec), dim3(CG_THREADS), 0, st, a.m, rc<NR>(a.ctx.xw, r2), c.Minv, rv<NR>(c.x, c2.x), rv<NR>(c.p, c2.p),
                           rv<NR>(c.slots_v, c2.slots_v));
    hipLaunchKernelGGL(k_cg_init_scalars<NR>, dim3(1), dim3(CG_THREADS), 0, st, sc, rc<NR>(c.slots_v, c2.slots_v), a.m > 0 ? c.geo.g_vec : 0, atol, rtol, (long long)itmax);
}
template <int NR>
int cg_iter(hipStream_t st, const DevArrays &a, const CgArrays &c, const CgArrays &c2, CgScalars *sc, const double *D, const double *regD, i64 k) {
    if (a.m <= 0) return 0;
    const int par = (int)(k & 1);
    double *const r2 = a.ctx.xw + a.ctx.xw2;
    int nl = 3;
    if (a.n > 0) {
        const unsigned gs = nblk(a.n * 4, CG_THREADS);
        hipLaunchKernelGGL(k_cg_cols<NR>, dim3(gs + (unsigned)c.geo.n_long_cols), dim3(CG_THREADS), 0, st, sc, a.n, a.Ap, a.Ai, a.Ax, D, rc<NR>(c.p, c2.p), rv<NR>(c.t, c2.t), gs,
                           c.geo.long_cols);
        ++nl;
    }
    hipLaunchKernelGGL(k_cg_rows<NR>, dim3((unsigned)(c.geo.g_rows + c.geo.g_lrows)), dim3(CG_ROW_THREADS), 0, st, sc, a.m, a.Tp, a.Tj, a.Tx, rc<NR>(c.t, c2.t), regD,
                       rc<NR>(c.p, c2.p), rv<NR>(c.q, c2.q), rv<NR>(c.slots_r, c2.slots_r), (unsigned)c.geo.g_rows, (unsigned)c.geo.g_lrows, c.geo.long_rows, c.geo.n_long_rows);
    hipLaunchKernelGGL(k_cg_step<NR>, dim3((unsigned)c.geo.g_vec), dim3(CG_THREADS), 0, st, sc, par, a.m, rv<NR>(c.x, c2.x), rv<NR>(a.ctx.xw, r2), rc<NR>(c.p, c2.p),
                       rc<NR>(c.q, c2.q), c.Minv, rc<NR>(c.slots_r, c2.slots_r), c.geo.g_rows + c.geo.g_lrows, rv<NR>(c.slots_v, c2.slots_v));
    hipLaunchKernelGGL(k_cg_dir<NR>, dim3((unsigned)c.geo.g_vec), dim3(CG_THREADS), 0, st, sc, par, (long long)k, a.m, rc<NR>(a.ctx.xw, r2), c.Minv, rv<NR>(c.p, c2.p),
                       rc<NR>(c.slots_v, c2.slots_v), c.geo.g_vec);
    return nl;
}

}  // namespace

void launch_cg_jacobi(hipStream_t st, const DevArrays &a, const CgArrays &c, const double *D, const double *regD) {
    if (a.m <= 0 || !c.Minv) return;
    const unsigned gs = nblk(a.m * 8, CG_THREADS);
    hipLaunchKernelGGL(k_cg_jacobi, dim3(gs + (unsigned)c.geo.n_long_rows), dim3(CG_THREADS), 0, st, a.m, a.Tp, a.Tj, a.Tx, D, regD, c.Minv, gs, c.geo.long_rows);
}

void launch_cg_init(hipStream_t st, const DevArrays &a, const CgArrays &c, double atol, double rtol, i64 itmax, const CgArrays *c2) {
    if (c2) cg_init<2>(st, a, c, *c2, c2->sc, atol, rtol, itmax);
    else cg_init<1>(st, a, c, c, c.sc, atol, rtol, itmax);
}

int launch_cg_iter(hipStream_t st, const DevArrays &a, const CgArrays &c, const double *D, const double *regD, i64 k, const CgArrays *c2) {
    return c2 ? cg_iter<2>(st, a, c, *c2, c2->sc, D, regD, k) : cg_iter<1>(st, a, c, c, c.sc, D, regD, k);
}

}  // namespace tlpk
