// tlpk_ipm.hpp -- device-resident interior-point state: views shared by
// ipm_kernels.hip and tlpk_ipm.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tlpk_host.hpp"

namespace tlpk {

constexpr int IPM_SLOTS = 16;      // reduction results per kernel
constexpr int IPM_BLOCKS = 1024;   // workgroups of the grid-stride kernels (per-block partials, fixed combination order)

// search direction (or any vector of the iterate's shape)
struct IpmDir { double *x, *xl, *xu, *zl, *zu /* n */, *y /* m */; };

// everything the kernels read; passed by value
struct IpmVecs {
    i64 m, n;
    const i64 *Ap; const i32 *Ai; const double *Ax;       // A, CSC (the handle's copy)
    const i64 *Tp; const i32 *Tj; const double *Tx;       // A, CSR
    const double *b, *c, *lz, *uz, *lflag, *uflag;        // problem data: l .* lflag, u .* uflag, flags as 0 / 1
    double *x, *xl, *xu, *zl, *zu, *y;                    // the iterate (point.jl)
    double *rp, *rl, *ru, *rd;                            // residuals (HSD.jl:83-110)
    double *thl, *thu;                                    // zl ./ xl, zu ./ xu on bounded entries
    double *hx, *hy;                                      // solution of the h-system (step.jl:56-66)
    double *hxid;                                         // its right-hand side c - th_l lz - th_u uz (own vector: the h-system and the
                                                          // predictor are solved as a pair, tlpk_ipm_hsolve_newton)
    double *xil, *xiu, *xzl, *xzu, *xid, *xip;            // right-hand sides of the current Newton system
    const double *aty, *ax;                               // dense-matrix handles (A is not stored as CSC / CSR: Ap ... Tx are null): A'y (n) and A x (m), formed by
                                                          // k_dense_gemv_t / k_dense_gemv_n in front of the kernels that need them; else nullptr
    const char *row_skip;                                 // shard of a multi-device handle: 1 on the linking rows (partial sums there: no part in the maxima); else nullptr
};

void ipm_launch_init(hipStream_t st, const IpmVecs &v);
void ipm_launch_finalize(hipStream_t st, int nblocks, int nsum, int nmax, int nmin, const double *partials, double *out);
int ipm_launch_res_cols(hipStream_t st, const IpmVecs &v, double tau, double *partials);
int ipm_launch_res_rows(hipStream_t st, const IpmVecs &v, double tau, double *partials);
void ipm_launch_theta(hipStream_t st, const IpmVecs &v, double *theta, double *regP, double *regD, double rP, double rD);
void ipm_launch_hrhs(hipStream_t st, const IpmVecs &v);
int ipm_launch_hdots(hipStream_t st, const IpmVecs &v, double *partials);
int ipm_launch_targets(hipStream_t st, const IpmVecs &v, const IpmDir &D, double a_p, double a_d, double mu_l, double mu_u, double *partials);
int ipm_launch_newton_pre(hipStream_t st, const IpmVecs &v, const IpmDir &D, int mode, double eta, double gmu, double delta, double *partials);
void ipm_launch_newton_dots(hipStream_t st, const IpmVecs &v, const IpmDir &D, int nblocks, double *partials);
int ipm_launch_newton_post(hipStream_t st, const IpmVecs &v, const IpmDir &D, const IpmDir &Add, int add, double dtau, double *partials);
int ipm_launch_advance(hipStream_t st, const IpmVecs &v, const IpmDir &D, double alpha_p, double alpha_d, double *partials);
void mpc_launch_fill(hipStream_t st, const IpmVecs &v, double *theta, double *regP, double *regD);
int mpc_launch_start(hipStream_t st, const IpmVecs &v, int stage, double a, double b, double *partials);
int mpc_launch_gap(hipStream_t st, const IpmVecs &v, const IpmDir &D, double ap, double ad, double *partials);

// ---- a stack of LPs on one handle (tlpk_ipm_load_batch, ipm_batch_kernels.hip) ----
// LP k owns the rows [row_off[k], row_off[k + 1]) and the columns [col_off[k], col_off[k + 1]) of the stacked vectors.  Every workgroup works inside one LP:
// a block table maps blockIdx.x to (LP, block within the LP); LP k has the blocks [first[k], first[k + 1]) -- as many as the unbatched kernel launches for a
// vector of the LP's length -- and its partials are the rows [first[k], first[k + 1]) of partials[block][slot].
constexpr int IPM_BSC = 8;         // scalars per LP and call; the last one is the LP's `active` flag (0.0 / 1.0)
struct IpmBlockTab { int nblocks; const int *seg, *loc, *first /* nlp + 1 */; };
struct IpmBatch {
    i64 nlp;
    const i64 *row_off, *col_off;          // nlp + 1 each
    IpmBlockTab tc, tr, tb;                // blocks sized by the LP's columns / rows / the longer of the two
    const double *sc;                      // nlp x IPM_BSC, uploaded per call
};
// blocks of one LP's segment of `len` entries: what ipm_kernels.hip launches for a vector of that length
inline int ipm_seg_blocks(i64 len) { return (int)std::max<i64>(1, std::min<i64>(IPM_BLOCKS, (len + 255) / 256)); }

void ipmb_launch_finalize(hipStream_t st, const IpmBatch &B, const IpmBlockTab &t, int nsum, int nmax, int nmin, const double *partials, double *out);
void ipmb_launch_init(hipStream_t st, const IpmVecs &v, const IpmBatch &B);      // the starting point of the LPs whose flag is set (tlpk_ipm_batch_refill)
void ipmb_launch_res_cols(hipStream_t st, const IpmVecs &v, const IpmBatch &B, double *partials);
void ipmb_launch_res_rows(hipStream_t st, const IpmVecs &v, const IpmBatch &B, double *partials);
void ipmb_launch_theta(hipStream_t st, const IpmVecs &v, const IpmBatch &B, double *theta, double *regP, double *regD);
void ipmb_launch_hrhs(hipStream_t st, const IpmVecs &v, const IpmBatch &B);
void ipmb_launch_hdots(hipStream_t st, const IpmVecs &v, const IpmBatch &B, double *partials);
void ipmb_launch_targets(hipStream_t st, const IpmVecs &v, const IpmDir &D, const IpmBatch &B, double *partials);
void ipmb_launch_newton_pre(hipStream_t st, const IpmVecs &v, const IpmDir &D, const IpmBatch &B, int mode, double *partials);
void ipmb_launch_newton_dots(hipStream_t st, const IpmVecs &v, const IpmDir &D, const IpmBatch &B, double *partials);
void ipmb_launch_newton_post(hipStream_t st, const IpmVecs &v, const IpmDir &D, const IpmDir &Add, const IpmBatch &B, int add, double *partials);
void ipmb_launch_advance(hipStream_t st, const IpmVecs &v, const IpmDir &D, const IpmBatch &B, double *partials);
void ipmb_launch_accept(hipStream_t st, const IpmDir &dst, const IpmDir &src, const IpmBatch &B);
void ipmb_launch_take(hipStream_t st, double *dx, double *dy, const double *sx, const double *sy, const IpmBatch &B);
// Mehrotra on a stack: fill / start stages 1 .. 4 / gap as mpc_launch_*; targets and advance with separate primal and dual lengths
// (B.sc of the call: start2 dxs | start3 dzs | start4 ddx, ddz | gap ap, ad | targets ap_, ad_, tmin, tmax | advance ap, ad)
void mpcb_launch_fill(hipStream_t st, const IpmVecs &v, const IpmBatch &B, double *theta, double *regP, double *regD);
void mpcb_launch_start(hipStream_t st, const IpmVecs &v, const IpmBatch &B, int stage, double *partials);
void mpcb_launch_gap(hipStream_t st, const IpmVecs &v, const IpmDir &D, const IpmBatch &B, double *partials);
void mpcb_launch_targets(hipStream_t st, const IpmVecs &v, const IpmDir &D, const IpmBatch &B, double *partials);
void mpcb_launch_advance(hipStream_t st, const IpmVecs &v, const IpmDir &D, const IpmBatch &B, double *partials);
// Mehrotra stream (tlpk_mpc_batch_*_enter): an LP that ENTERS a slot gets its starting point from the update and the two solves the running LPs need anyway.
// The role of LP k in the call travels in B.sc[k][IPM_ROLE]; an entering LP's `active` flag is 0, so every kernel above skips it.
constexpr int IPM_ROLE = IPM_BSC - 2;
constexpr double IPM_PARKED = 0.0, IPM_ACTIVE = 1.0, IPM_ENTERING = 2.0;
// theta / regP / regD by role: active as ipmb_launch_theta (sc[0] = regP, sc[1] = regD), parked as it parks, entering as mpcb_launch_fill
void mpcb_launch_theta_enter(hipStream_t st, const IpmVecs &v, const IpmBatch &B, double *theta, double *regP, double *regD);
// ... and with a fourth role (tlpk_ipm_batch_factor_each): an LP that holds its factor keeps its segments of theta / regP / regD untouched
constexpr double IPM_HOLD = 3.0;
void ipmb_launch_theta_roles(hipStream_t st, const IpmVecs &v, const IpmBatch &B, double *theta, double *regP, double *regD);
// entering LPs only.  mode 0: (xip, xid) = (0, c), the solution goes to (D0.x, y); mode 1: (xip, xid) = (b, 0), the solution goes to (x, D0.y).
// The take puts the half of the right-hand side it used back to 0, as tlpk_mpc_batch_start leaves it.
void mpcb_launch_enter_rhs(hipStream_t st, const IpmVecs &v, const IpmBatch &B, int mode);
void mpcb_launch_enter_take(hipStream_t st, const IpmVecs &v, const IpmDir &D0, const double *sx, const double *sy, const IpmBatch &B, int mode);
// tlpk_ipm_get_lps: segment s of the table is copied to out + dst; blockIdx.x = segment, blockIdx.y strides within it
struct IpmGatherSeg { const double *src; i64 len, dst; };
void ipmb_launch_gather_segs(hipStream_t st, const IpmGatherSeg *tab, i64 nseg, i64 maxlen, double *out);

}  // namespace tlpk
