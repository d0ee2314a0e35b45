// ipm_shared.hpp -- what ipm_kernels.hip (one LP per handle) and ipm_batch_kernels.hip (a stack of LPs, one segment each) share:
// the workgroup size, the fixed LDS reduction trees and the per-entry bodies of the homogeneous self-dual kernels.  A kernel of
// either file is a grid-stride loop around one of these bodies -- over the whole vector, or over one LP's range with that LP's
// scalars -- so the formulas exist once, and a one-LP batch is the unbatched loop bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "tlpk_ipm.hpp"

namespace tlpk {

constexpr int IPM_T = 256;

__device__ __forceinline__ double blk_sum(double v, double *sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = IPM_T / 2; s > 0; s >>= 1) { if (tid < s) sh[tid] += sh[tid + s]; __syncthreads(); }
    const double r = sh[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double blk_max(double v, double *sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = IPM_T / 2; s > 0; s >>= 1) { if (tid < s) sh[tid] = fmax(sh[tid], sh[tid + s]); __syncthreads(); }
    const double r = sh[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double blk_min(double v, double *sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = IPM_T / 2; s > 0; s >>= 1) { if (tid < s) sh[tid] = fmin(sh[tid], sh[tid + s]); __syncthreads(); }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// ---- per-entry bodies (citations into the reference: at the kernels of ipm_kernels.hip) ----
// column j of the starting point
__device__ __forceinline__ void ipm_init_col(const IpmVecs &v, i64 j) { v.x[j] = 0.0; v.xl[j] = v.lflag[j]; v.xu[j] = v.uflag[j]; v.zl[j] = v.lflag[j]; v.zu[j] = v.uflag[j]; }
// column j of the residuals: rl, ru, rd + sums {c'x, lz'zl, uz'zu, xl'zl + xu'zu} + maxima {|rl|, |ru|, |rd|, |(x-xl) lflag|, |(x+xu) uflag|, |A'y + zl - zu|}
__device__ __forceinline__ void ipm_res_col(const IpmVecs &v, i64 j, double tau, double &s0, double &s1, double &s2, double &s3,
                                            double &m0, double &m1, double &m2, double &m3, double &m4, double &m5) {
    double aty = 0.0;
    if (v.aty) aty = v.aty[j];
    else for (i64 p = v.Ap[j]; p < v.Ap[j + 1]; ++p) aty += v.Ax[p] * v.y[v.Ai[p]];
    const double x = v.x[j], xl = v.xl[j], xu = v.xu[j], zl = v.zl[j], zu = v.zu[j], lf = v.lflag[j], uf = v.uflag[j];
    const double rl = (-x + xl + tau * v.lz[j]) * lf, ru = (-x - xu + tau * v.uz[j]) * uf;
    const double rd = tau * v.c[j] - aty + zu * uf - zl * lf;
    v.rl[j] = rl; v.ru[j] = ru; v.rd[j] = rd;
    s0 += v.c[j] * x; s1 += v.lz[j] * zl; s2 += v.uz[j] * zu; s3 += xl * zl + xu * zu;
    m0 = fmax(m0, fabs(rl)); m1 = fmax(m1, fabs(ru)); m2 = fmax(m2, fabs(rd));
    m3 = fmax(m3, fabs((x - xl) * lf)); m4 = fmax(m4, fabs((x + xu) * uf)); m5 = fmax(m5, fabs(aty + zl * lf - zu * uf));
}
// row i of the residuals, by the 8 lanes of its group (every lane of the group calls it: the shuffles stay convergent; `live`: the row exists):
// rp + sum {b'y} + maxima {|rp|, |A x|}
__device__ __forceinline__ void ipm_res_row(const IpmVecs &v, i64 i, bool live, int lane, double tau, double &s0, double &m0, double &m1) {
    double ax = 0.0;
    if (live && v.ax) ax = (lane == 0) ? v.ax[i] : 0.0;
    else if (live)
        for (i64 q = v.Tp[i] + lane; q < v.Tp[i + 1]; q += 8) ax += v.Tx[q] * v.x[v.Tj[q]];
#pragma unroll
    for (int off = 4; off > 0; off >>= 1) ax += __shfl_down(ax, off, 8);
    if (!live || lane != 0) return;
    const double rp = tau * v.b[i] - ax;
    v.rp[i] = rp;
    s0 += v.b[i] * v.y[i];
    if (v.row_skip && v.row_skip[i]) return;                                // a shard's PARTIAL linking row: the host sums the shards' rows
    m0 = fmax(m0, fabs(rp)); m1 = fmax(m1, fabs(ax));
}
__device__ __forceinline__ void ipm_theta_col(const IpmVecs &v, i64 j, double *__restrict__ theta) {
    const double tl = (v.lflag[j] != 0.0) ? v.zl[j] / v.xl[j] : 0.0, tu = (v.uflag[j] != 0.0) ? v.zu[j] / v.xu[j] : 0.0;
    v.thl[j] = tl; v.thu[j] = tu; theta[j] = tl + tu;
}
__device__ __forceinline__ void ipm_hrhs_col(const IpmVecs &v, i64 j) { v.hxid[j] = v.c[j] - v.thl[j] * v.lz[j] - v.thu[j] * v.uz[j]; }
__device__ __forceinline__ void ipm_hdots_col(const IpmVecs &v, i64 j, double &s0) {
    const double lz = v.lz[j], uz = v.uz[j], tl = v.thl[j], tu = v.thu[j];
    s0 += lz * (lz * tl) + uz * (uz * tu) - (v.c[j] + tl * lz + tu * uz) * v.hx[j];
}
__device__ __forceinline__ void ipm_targets_col(const IpmVecs &v, const IpmDir &D, i64 j, double a_p, double a_d, double mu_l, double mu_u, double &s0, double &s1) {
    double vl = ((v.xl[j] + a_p * D.xl[j]) * (v.zl[j] + a_d * D.zl[j])) * v.lflag[j];
    double vu = ((v.xu[j] + a_p * D.xu[j]) * (v.zu[j] + a_d * D.zu[j])) * v.uflag[j];
    if (v.lflag[j] != 0.0) vl = (vl < mu_l) ? mu_l - vl : ((vl > mu_u) ? mu_u - vl : 0.0);
    if (v.uflag[j] != 0.0) vu = (vu < mu_l) ? mu_l - vu : ((vu > mu_u) ? mu_u - vu : 0.0);
    v.xzl[j] = vl; v.xzu[j] = vu;
    s0 += vl; s1 += vu;
}
__device__ __forceinline__ void ipm_newton_pre_col(const IpmVecs &v, const IpmDir &D, i64 j, int mode, double eta, double gmu, double delta,
                                                   double &s0, double &s1, double &s2, double &s3) {
    const double lf = v.lflag[j], uf = v.uflag[j], xl = v.xl[j], xu = v.xu[j], zl = v.zl[j], zu = v.zu[j];
    double xil, xiu, xd, xzl, xzu;
    if (mode == 0) { xil = v.rl[j]; xiu = v.ru[j]; xd = v.rd[j]; xzl = -(xl * zl) * lf; xzu = -(xu * zu) * uf; }
    else if (mode == 1) {
        xil = eta * v.rl[j]; xiu = eta * v.ru[j]; xd = eta * v.rd[j];
        xzl = (-xl * zl + gmu - D.xl[j] * D.zl[j]) * lf; xzu = (-xu * zu + gmu - D.xu[j] * D.zu[j]) * uf;
    } else { xil = 0.0; xiu = 0.0; xd = 0.0; xzl = v.xzl[j] - delta; xzu = v.xzu[j] - delta; }
    v.xil[j] = xil; v.xiu[j] = xiu; v.xzl[j] = xzl; v.xzu[j] = xzu;
    const double tl = (lf != 0.0) ? (xzl + zl * xil) / xl : 0.0, tu = (uf != 0.0) ? (xzu - zu * xiu) / xu : 0.0;
    v.xid[j] = xd - tl + tu;                                            // step.jl:214
    const double ixl = (lf != 0.0) ? xzl / xl : 0.0, ixu = (uf != 0.0) ? xzu / xu : 0.0;
    s0 += ixl * v.lz[j]; s1 += ixu * v.uz[j]; s2 += (v.thl[j] * xil) * v.lz[j]; s3 += (v.thu[j] * xiu) * v.uz[j];
}
__device__ __forceinline__ void ipm_newton_pre_row(const IpmVecs &v, i64 i, int mode, double eta) { v.xip[i] = (mode == 0) ? v.rp[i] : (mode == 1 ? eta * v.rp[i] : 0.0); }
__device__ __forceinline__ void ipm_newton_dots_col(const IpmVecs &v, const IpmDir &D, i64 j, double &s0) { s0 += (v.c[j] + v.thl[j] * v.lz[j] + v.thu[j] * v.uz[j]) * D.x[j]; }
__device__ __forceinline__ void ipm_newton_post_col(const IpmVecs &v, const IpmDir &D, const IpmDir &Add, i64 j, int add, double dtau, double &amin_p, double &amin_d) {
    const double lf = v.lflag[j], uf = v.uflag[j];
    double dx = D.x[j] + dtau * v.hx[j];
    double dxl = (-v.xil[j] + dx - dtau * v.lz[j]) * lf, dxu = (v.xiu[j] - dx + dtau * v.uz[j]) * uf;
    double dzl = (lf != 0.0) ? (v.xzl[j] - v.zl[j] * dxl) / v.xl[j] : 0.0, dzu = (uf != 0.0) ? (v.xzu[j] - v.zu[j] * dxu) / v.xu[j] : 0.0;
    if (add) { dx += Add.x[j]; dxl += Add.xl[j]; dxu += Add.xu[j]; dzl += Add.zl[j]; dzu += Add.zu[j]; }
    D.x[j] = dx; D.xl[j] = dxl; D.xu[j] = dxu; D.zl[j] = dzl; D.zu[j] = dzu;
    if (dxl < 0.0) amin_p = fmin(amin_p, -v.xl[j] / dxl);
    if (dxu < 0.0) amin_p = fmin(amin_p, -v.xu[j] / dxu);
    if (dzl < 0.0) amin_d = fmin(amin_d, -v.zl[j] / dzl);
    if (dzu < 0.0) amin_d = fmin(amin_d, -v.zu[j] / dzu);
}
__device__ __forceinline__ void ipm_newton_post_row(const IpmVecs &v, const IpmDir &D, const IpmDir &Add, i64 i, int add, double dtau) {
    double dy = D.y[i] + dtau * v.hy[i]; if (add) dy += Add.y[i]; D.y[i] = dy;
}
__device__ __forceinline__ void ipm_advance_col(const IpmVecs &v, const IpmDir &D, i64 j, double alpha, double alpha_d, double &s0) {
    v.x[j] += alpha * D.x[j];
    const double xl = v.xl[j] + alpha * D.xl[j], xu = v.xu[j] + alpha * D.xu[j], zl = v.zl[j] + alpha_d * D.zl[j], zu = v.zu[j] + alpha_d * D.zu[j];
    v.xl[j] = xl; v.xu[j] = xu; v.zl[j] = zl; v.zu[j] = zu;
    s0 += xl * zl + xu * zu;
}

// ---- Mehrotra predictor-corrector: the starting point (MPC.jl:365-405) and the complementarity after a trial step (MPC/step.jl:246-258) ----
// minima of (x - l) lflag and (u - x) uflag (entries without the bound contribute 0, as `false * Inf` does there)
__device__ __forceinline__ void mpc_start1_col(const IpmVecs &v, i64 j, double &m0, double &m1) {
    if (v.lflag[j] != 0.0) m0 = fmin(m0, v.x[j] - v.lz[j]);
    if (v.uflag[j] != 0.0) m1 = fmin(m1, v.uz[j] - v.x[j]);
}
// xl, xu shifted by dxs; z = c - A'y split over the finite bounds; minima of zl, zu
__device__ __forceinline__ void mpc_start2_col(const IpmVecs &v, i64 j, double dxs, double &m0, double &m1) {
    const double lf = v.lflag[j], uf = v.uflag[j], x = v.x[j];
    v.xl[j] = (lf != 0.0) ? (x - v.lz[j]) + dxs : 0.0;
    v.xu[j] = (uf != 0.0) ? (v.uz[j] - x) + dxs : 0.0;
    double aty = 0.0;
    if (v.aty) aty = v.aty[j];
    else for (i64 p = v.Ap[j]; p < v.Ap[j + 1]; ++p) aty += v.Ax[p] * v.y[v.Ai[p]];
    const double z = v.c[j] - aty, nb = lf + uf;
    const double zl = (lf != 0.0) ? z / nb : 0.0, zu = (uf != 0.0) ? -z / nb : 0.0;
    v.zl[j] = zl; v.zu[j] = zu;
    m0 = fmin(m0, zl); m1 = fmin(m1, zu);
}
// zl, zu shifted by dzs; sums {xl'zl + xu'zu, sum zl + sum zu, sum xl + sum xu}
__device__ __forceinline__ void mpc_start3_col(const IpmVecs &v, i64 j, double dzs, double &s0, double &s1, double &s2) {
    const double zl = (v.lflag[j] != 0.0) ? v.zl[j] + dzs : v.zl[j], zu = (v.uflag[j] != 0.0) ? v.zu[j] + dzs : v.zu[j];
    v.zl[j] = zl; v.zu[j] = zu;
    const double xl = v.xl[j], xu = v.xu[j];
    s0 += xl * zl + xu * zu; s1 += zl + zu; s2 += xl + xu;
}
// balanced products: xl, xu += ddx, zl, zu += ddz on the finite bounds; sum xl'zl + xu'zu
__device__ __forceinline__ void mpc_start4_col(const IpmVecs &v, i64 j, double ddx, double ddz, double &s0) {
    double xl = v.xl[j], xu = v.xu[j], zl = v.zl[j], zu = v.zu[j];
    if (v.lflag[j] != 0.0) { xl += ddx; zl += ddz; }
    if (v.uflag[j] != 0.0) { xu += ddx; zu += ddz; }
    v.xl[j] = xl; v.xu[j] = xu; v.zl[j] = zl; v.zu[j] = zu;
    s0 += xl * zl + xu * zu;
}
// {((xl + ap dxl) lflag)'(zl + ad dzl) + ((xu + ap dxu) uflag)'(zu + ad dzu), xl'zl + xu'zu}
__device__ __forceinline__ void mpc_gap_col(const IpmVecs &v, const IpmDir &D, i64 j, double ap, double ad, double &s0, double &s1) {
    const double xl = v.xl[j], xu = v.xu[j], zl = v.zl[j], zu = v.zu[j];
    s0 += ((xl + ap * D.xl[j]) * v.lflag[j]) * (zl + ad * D.zl[j]) + ((xu + ap * D.xu[j]) * v.uflag[j]) * (zu + ad * D.zu[j]);
    s1 += xl * zl + xu * zu;
}

}  // namespace tlpk
