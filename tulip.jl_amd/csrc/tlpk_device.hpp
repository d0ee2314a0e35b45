// tlpk_device.hpp -- device-side views shared by kernels.hip and tlpk_api.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include "tlpk_host.hpp"

namespace tlpk {

// passed by value to every front kernel
struct DevCtx {
    const FrontDesc *fronts;
    const i32 *rowidx;
    const i32 *rel;
    const i32 *ea_tab;  // extend-add lookup (FrontDesc.eatab)
    const i32 *children;
    const i64 *gth_ptr, *gth_src;   // forward gather lists (per front row: the children's uc entries)
    double *Lval;       // supernodal panels of L
    double *U0, *U1;    // ping-pong update-matrix buffers (by tree depth parity)
    double *uc;         // solve contribution vectors
    double *xw;         // permuted right-hand side / solution
    double *dinv;       // inverses of the NB_IN x NB_IN diagonal blocks of L (written by k_potrf)
    double *spart;      // split-K scratch: one TILE x TILE partial product per slot
    int *info;          // info[0] = smallest failing pivot column (INT_MAX = none); info[1] != 0: a sweep gave up waiting; info[INFO_WORDS + col] = col for every
                        // column that info[0] was offered (kernels.hip: record_fail) -- the marks the per-LP pivot verdicts are folded from
    int upd_remap;         // k_update blockIdx -> task mapping (0 identity, 1 XCD-contiguous, 2 runs of 64 tasks per XCD)
    const double *csign;   // K2 (augmented system): +1 / -1 per permuted column, the S of P K P' = L S L'; nullptr for K1
    const i32 *upd_seg;    // K-segment lists of the update tasks (UpdateTask.seg)
    int small_full;        // TLPK_SMALL_FULL=1 (debugging): the small-front solve kernels always take their (16 columns, 256 rows) body
    i64 xw2, uc2;          // two-right-hand-side solves: the second rhs / solution at xw + xw2, its contribution vectors at uc + uc2
    // per-column extend-add index (k_ea_gather): eg_front == nullptr: none; else != 0 per front whose extend-add k_ea_gather does (k_extend_add leaves its
    // tasks alone); eg_col + eg_base[front] = per column of the front its first segment (eg_cap rows each), eg_ptr[segment] = its first entry of eg_ent
    const unsigned char *eg_front; const i64 *eg_base, *eg_col, *eg_ptr; const EaGatherEnt *eg_ent; i32 eg_cap;
    // Bit 1 of a front's byte (EG_FORMED): the front is FORMED (Symbolic::ea_form) -- its panel is not zero-filled, k_ea_gather<true> writes every stored double
    // of its columns.  (In this byte and not in a field of its own: DevCtx is an argument of every front kernel, and three more pointers in it moved k_chain's
    // scratch from 500 to 532 bytes per lane; the index of the formed fronts is an argument of the one kernel that reads it, DevArrays::eg_asm_*.)
    const unsigned char *front_skip;  // block skip (tlpk_block_skip / tlpk_ipm_batch_skip): nullptr = no mask; else != 0 per front (then per single) that this update / solve leaves out
};
constexpr unsigned char EG_GATHERED = 1, EG_FORMED = 2;   // bits of DevCtx::eg_front[front]
constexpr int INFO_WORDS = 16;  // status and diagnostic words of DevCtx.info, in front of its m mark words

// per-launch arguments of the persistent sweep kernels
struct SweepArgs {
    unsigned long long *ticket;   // hand-out counter of this launch: reset to all ones with the hand-over words (ONE memset per solve covers
                                  // both), so that atomicAdd(ticket, 1) + 1 hands out 0, 1, 2, ... -- no per-launch host state in the kernel
                                  // arguments: the solve schedule can be replayed from a captured graph
    double *xh;                   // hand-over words of this direction, one per permuted column, sentinel-filled before the solve
    i64 xh2;                      // ... of the second right-hand side at xh + xh2 (two-rhs sweeps)
    int poll_fast, poll_nfast, poll_slow;   // polling back-off (units of s_sleep 1 = 64 clocks): first poll_nfast polls every poll_fast, then every poll_slow
    const SolveTask *small = nullptr;       // round 6: the small-front tasks of this direction (items with slot == 2 of a merged launch name groups of four of them)
};

// an LK_EXTEND_ADD launch as its two kernels see it, counted at create (tlpk_api.cpp: eg_count_launches): tasks of k_ea_gather / of k_extend_add,
// rows of a wave's LDS slice = the longest segment k_ea_gather holds in the launch; n_form of the n_gather tasks are panel-part tasks of formed fronts
// [s0, s1): the launch's records of the flat segment list (Symbolic::ea_seg; empty range: its formed panel tasks, if any, stay on k_ea_gather<true>)
struct EaGatherLaunch { i64 first; i32 n_gather, n_plain, rows, n_form; i64 s0 = 0, s1 = 0; };
// consecutive records of that list per wave of k_ea_seglist (measured on C4: 4, 8, 16 and 32 within the noise of each other)
constexpr int EG_SEG_CHUNK = 8;

struct DevArrays {
    DevCtx ctx{};
    const EaGatherLaunch *eg_launch = nullptr; i64 n_eg_launch = 0;   // host memory of the handle, ascending `first`; nullptr: no front is gathered
    // formed fronts (Symbolic::ea_gather_asm_*): eg_asm_row[eg_asm_ptr[segment] ..] = the rows, from the segment's first row, of the entries k_assemble stores in it
    const i64 *eg_asm_ptr = nullptr; const unsigned short *eg_asm_row = nullptr;
    // flat segment list of the formed fronts' panel columns (TLPK_EA_SEGLIST; Symbolic::ea_seg): an argument of k_ea_seglist, like eg_asm_* not a field of
    // DevCtx; nullptr: k_ea_gather<true> does them
    const EaSeg *eg_seg = nullptr;
    i64 m = 0, n = 0;                         // m: order of the factored matrix (K2: n + m; dense columns: m + k), n: columns of the stored matrix
    i64 mu = 0;                               // rows of A as the caller sees them (= m for plain K1): the residual kernels of the refinement
    // K1 with dense columns (tlpk_options.dense_cols): sparse_col[j] = 1 for a column formed into A_s D_s A_s', 0 for a dense one;
    // dense_col[t] = the column of node mu + t
    char *sparse_col = nullptr; i32 *dense_col = nullptr; i64 n_dense = 0;
    // dense-matrix handle (tlpk_create_dense): A column-major with leading dimension dlda (tlpk_host.hpp: dense_lda), padding rows zero; then the
    // CSC / CSR arrays below and the assembly lists stay null.  Launch geometry of the dense kernels from analyse_dense_matrix
    const double *dA = nullptr; i64 dlda = 0;
    i32 syrk_split = 1; i64 syrk_kc = 0;
    double *gemv_part = nullptr; i64 gemv_chunks = 0, gemv_cw = 0;      // k_dense_gemv_n: [2][chunks][dlda] partial sums
    // A (CSC + CSR)
    i64 *Ap = nullptr; i32 *Ai = nullptr; double *Ax = nullptr;
    i64 *Tp = nullptr; i32 *Tj = nullptr; double *Tx = nullptr;
    i32 *perm = nullptr;
    i64 *Pp = nullptr; i32 *Pj = nullptr; double *Px = nullptr;   // K1: CSR of A with the rows in permuted order (k_rhs)
    double *rhs_w = nullptr;                  // D .* xi_d of the current solve (k_rhs_scale)
    i32 *zero_tasks = nullptr; i64 n_zero_tasks = 0;   // (front, c0) pairs of k_zero_panels
    i64 n_zero_lower = 0;                              // the first n_zero_lower pairs: fronts that are not `upper` (schedule.cpp, step 13d)
    unsigned char *asm_upper = nullptr; bool has_upper = false;   // per assembled entry: 1 = its front is upper
    i32 *zero_small = nullptr; i64 n_zero_small = 0;   // fronts zeroed whole, one wave each
    char *row_local = nullptr, *col_local = nullptr;
    // assembly lists (local entries only)
    i64 n_asm = 0;
    i64 *asm_target = nullptr; i32 *asm_diag = nullptr; i64 *asm_ptr = nullptr;
    double *pair_w = nullptr; i32 *pair_j = nullptr;
    // task arrays
    FaTask *fa_tasks = nullptr;              // k_front_assemble tiles
    i64 *asm_colptr = nullptr;               // per permuted column: first entry of the (compacted) assembly list; k_front_assemble walks the columns of its tile
    i64 *asm_target_small = nullptr;         // asm_target with -1 for the entries k_front_assemble forms: what k_assemble writes
    const double *asm_D = nullptr, *asm_regD = nullptr;   // handle-owned D = 1 / (theta + regP) (K2: D2) and regD, read by the assembly kernels
    EaTask *ea_tasks = nullptr; PotrfTask *potrf_tasks = nullptr; TrsmTask *trsm_tasks = nullptr;
    UpdateTask *update_tasks = nullptr, *reduce_tasks = nullptr;
    ChainItem *chain_items = nullptr;                 // items of the LK_CHAIN launches (k_chain)
    unsigned long long *chain_trace = nullptr;        // TLPK_CHAIN_TRACE=1: 4 time stamps per item (kernels.hip: k_chain), read back through tlpk_symbolic_get("chain_trace")
    unsigned *chain_cnt = nullptr; i64 n_chain_cnt = 0;   // their tickets + completion counters, zeroed at the start of every update
    i64 n_single = 0; i64 *single_loff = nullptr, *single_dinvoff = nullptr; i32 *single_col = nullptr;   // isolated 1 x 1 fronts
    SolveTask *fwd_gather_tasks = nullptr, *fwd_diag_tasks = nullptr, *fwd_update_tasks = nullptr,
              *bwd_update_tasks = nullptr, *fwd_small_tasks = nullptr, *bwd_small_tasks = nullptr,
              *fwd_sweep_tasks = nullptr, *bwd_sweep_tasks = nullptr;
    unsigned long long *sweep_tickets = nullptr;      // one counter per sweep launch of the schedules, stored right in front of ...
    double *sweep_xh = nullptr;                       // ... the hand-over words: [0, m) forward sweep, [m, 2m) backward sweep
    i64 sweep_reset_bytes = 0, sweep_reset_bytes2 = 0;   // tickets + hand-over words (of one / two right-hand sides): one hipMemsetAsync(0xFF) per solve
    // block skip, allocated by the first mask (tlpk_api.cpp: skip_tables): unit of every front and then of every single; the front of every assembled entry
    // (k_assemble works per entry); the storage ctx.front_skip points at while a mask is in force; the per-unit bytes of tlpk_block_skip
    i64 n_fronts = 0;
    i32 *front_unit = nullptr, *asm_front = nullptr;
    unsigned char *skip_bytes = nullptr, *unit_skip = nullptr;
    // per-LP pivot verdicts, allocated by the first tlpk_ipm_batch_factor_each: the LP of every permuted column; the smallest marked column per LP (FAIL_NONE:
    // none), written by k_fold_fail after an update that failed.  The marks themselves are the m words behind ctx.info's first INFO_WORDS, set to FAIL_NONE before the update
    int *unit_fail = nullptr; i32 *col_unit = nullptr;
};
constexpr int FAIL_NONE = 0x7f7f7f7f;   // (what hipMemsetAsync(0x7f) leaves: above every column)

void launch_compute_d(hipStream_t st, i64 n, const double *theta, const double *regP, double *D);
// part: -1 = everything, 0 = the lower fronts only, 1 = the upper fronts only (schedule.cpp, step 13d)
void launch_assemble(hipStream_t st, const DevArrays &a, const double *D, const double *regD, int part = -1);
void launch_zero_panels(hipStream_t st, const DevArrays &a, int part = -1);
void launch_tasks(hipStream_t st, const DevArrays &a, const Launch &L, const SweepArgs *sw = nullptr, int nrhs = 1);
void launch_single_factor(hipStream_t st, const DevArrays &a);
// a.skip_bytes from the units' bytes (unit_skip, != 0 = skipped) or from the units' flags (unit_active[k * stride], 0.0 = skipped); one of the two is null
void launch_expand_skip(hipStream_t st, const DevArrays &a, const unsigned char *unit_skip, const double *unit_active, int stride);
// a.unit_fail[u] = the smallest marked column of unit u (a.unit_fail holds FAIL_NONE before)
void launch_fold_fail(hipStream_t st, const DevArrays &a);
// The per-right-hand-side kernels of a solve: nrhs = 1, or 2 for a pair (ONE launch each where the kernel has a grid-y form, grid y = right-hand side; slots
// 0 .. nrhs - 1 of xw); the pointer arrays hold nrhs entries.  dy_shared / local_only: shards of a multi-device handle publishing into the lead's vectors (nrhs = 1)
void launch_single_solve(hipStream_t st, const DevArrays &a, int nrhs = 1);
void launch_rhs(hipStream_t st, const DevArrays &a, const double *D, const double *const *xi_p, const double *const *xi_d, int rank, int nrhs);
void launch_unpermute(hipStream_t st, const DevArrays &a, double *const *dy, double *dy_shared, int rank, int nrhs);
void launch_dx(hipStream_t st, const DevArrays &a, const double *D, double *const *dy, const double *const *xi_d, double *const *dx, int local_only, int nrhs);
void launch_residuals(hipStream_t st, const DevArrays &a, const double *xi_p, const double *xi_d, const double *theta, const double *regP,
                      const double *regD, const double *dx, const double *dy, double *r1, double *r2, int rank, int xip_all = 0);
void launch_publish(hipStream_t st, const DevArrays &a, const double *dx, double *dx_job, const double *dy, double *dy_job);
void launch_axpy2(hipStream_t st, i64 n, double *x, const double *dxc, i64 m, double *y, const double *dyc);
// guarded refinement (kernels.hip: k_absmax2 ...): max-norm of (r1, r2) into *out (bit pattern, atomicMax: zero it first), verdict, candidate, commit
void launch_absmax2(hipStream_t st, const DevArrays &a, const double *r1, const double *r2, unsigned long long *out, int owned_only = 0);
void launch_refine_decide(hipStream_t st, unsigned long long *ref);
void launch_candidate(hipStream_t st, i64 n, const double *x, double *cx, i64 m, const double *y, double *cy);
void launch_refine_commit(hipStream_t st, i64 n, double *x, const double *cx, i64 m, double *y, const double *cy, const unsigned long long *ref);
// refinement on demand (refine_kernels.hip; tlpk_polish_device / tlpk_polish2_device): A as the caller sees it (K2: the copies built by the first
// call), the vectors of one or two systems (slot 1 repeats slot 0 for one), and the state words of a system -- PW of them, system r at ref + r * PW:
// bit patterns of non-negative doubles (PW_R1: |r1| of the kept iterate, PW_R2_REF: |r2| at entry, PW_C1 / PW_C2: of the candidate, PW_R1_IN: |r1| at
// entry, PW_R2_KEPT: |r2| of the kept iterate), PW_STATE = {int rejected, int stop}, PW_ACCEPT = {int verdict of the last step, int accepted steps}
struct PolishMat { i64 m, n; const i64 *Ap; const i32 *Ai; const double *Ax; const i64 *Tp; const i32 *Tj; const double *Tx; };
struct PolishVecs { const double *xi_p[2], *xi_d[2], *dx[2], *dy[2]; double *r1[2], *r2[2]; };
struct PolishPair { double *x[2], *y[2], *cx[2], *cy[2]; };
enum : int { PW_R1 = 0, PW_R2_REF = 1, PW_C1 = 2, PW_C2 = 3, PW_STATE = 4, PW_ACCEPT = 5, PW_R1_IN = 6, PW_R2_KEPT = 7, PW = 8 };
// residuals of nr systems in one pass over A, with their max-norms: entry != 0 -> the norms of the iterate a call starts from, else the candidate's
void launch_kkt_resid(hipStream_t st, const PolishMat &A, const double *theta, const double *regP, const double *regD, const PolishVecs &v,
                      unsigned long long *ref, int nr, int entry);
void launch_polish_decide(hipStream_t st, unsigned long long *ref, int nr);
void launch_polish_candidate(hipStream_t st, i64 n, i64 m, const PolishPair &p, int nr);
void launch_polish_commit(hipStream_t st, i64 n, i64 m, const PolishPair &p, const unsigned long long *ref, int nr);
void launch_sum_to(hipStream_t st, i64 len, double *out, const double *own, const double *src, int nsrc, i64 stride);
void launch_sum_ranked(hipStream_t st, i64 len, double *inout, const double *stage, int nranks, int own_rank, i64 stride);
void launch_k2_diag(hipStream_t st, i64 n, const double *theta, const double *regP, double *D2);
void launch_k2_rhs(hipStream_t st, const DevArrays &a, i64 n, const double *const *xi_p, const double *const *xi_d, int rank, int nrhs);
void launch_apply_signs(hipStream_t st, const DevArrays &a, int nrhs);
void launch_k2_out(hipStream_t st, const DevArrays &a, i64 n, double *const *dx, double *const *dy, int rank, int owned_only, int nrhs);
// K1 with dense columns (kernels.hip: k_dense_*): D = [sparse j: 1 / (theta + regP), dense j: theta + regP ; 1]; the permuted right-hand side
// [xi_p + A_s D_s xi_d_s ; xi_d_d]; [dy ; dx_d] = P' x and dx_s = D_s (A_s' dy - xi_d_s).  nrhs = 2: both right-hand sides of a pair in one
// launch each (grid y), slots 0 / 1 of xw -- the same arithmetic per right-hand side as two single solves
void launch_dense_diag(hipStream_t st, const DevArrays &a, const double *theta, const double *regP, double *D);
void launch_dense_rhs(hipStream_t st, const DevArrays &a, const double *D, const double *const *xi_p, const double *const *xi_d, int nrhs);
void launch_dense_out(hipStream_t st, const DevArrays &a, const double *D, double *const *dy, const double *const *xi_d, double *const *dx, int nrhs);
// dense-matrix handles (dense_kernels.hip).  S = A diag(D) A' + diag(regD), lower triangle, into the packed panel P (leading dimension plda)
void launch_dense_syrk(hipStream_t st, const DevArrays &a, const double *D, const double *regD, double *P, i32 plda);
// out[r] = add[r] + A (D .* x[r])  (D, add[r] may be null), r < nrhs <= 2: one pass over A
void launch_dense_gemv_n(hipStream_t st, const DevArrays &a, const double *D, const double *const *x, const double *const *add, double *const *out, int nrhs);
// out[r] = D .* (A' y[r] - xi_d[r])  (D null: A' y[r]), r < nrhs <= 2: one pass over A
void launch_dense_gemv_t(hipStream_t st, const DevArrays &a, const double *D, const double *const *y, const double *const *xi_d, double *const *out, int nrhs);

// ---- matrix-free handles (tlpk_options.krylov).  K1: conjugate gradients on (A D A' + Rd) dy = b (krylov_kernels.hip; DESIGN.md section 1b'''') ----
// The scalars of a solve, in device memory: read by every kernel, written by ONE thread of the kernel that owns the field.  The host copies the block to
// pinned memory after every chunk of iterations.
struct CgScalars {
    double gamma[2];      // r' M^-1 r, by parity of the iteration that READS it (iteration k reads gamma[k & 1] and writes gamma[(k + 1) & 1])
    double tol;           // atol + rtol sqrt(gamma at x = 0)
    double resid0, resid; // sqrt(gamma) at x = 0 / after the last completed iteration
    double pq;            // the last p' S p
    long long outcome;    // CG_RUNNING until a kernel decides; every kernel returns at once when it is set
    long long iters;      // completed iterations
    long long itmax;
    long long pad[7];
};
static_assert(sizeof(CgScalars) == 128, "CgScalars layout");
enum : long long { CG_RUNNING = 0, CG_SOLVED = 1, CG_ITMAX = 2, CG_BREAKDOWN = 3 };
constexpr int CG_LONG = 512;        // a row / column with more entries gets a workgroup of its own (binned at create); shorter ones 8 / 4 lanes
constexpr int CG_MAX_SLOTS = 256;   // workgroups (= partial sums) of the short rows / of the vector kernels
constexpr int CG_MAX_LONG = 64;     // workgroups that share the long rows
// The lists of the long rows / columns and the launch geometry, shared by the three methods and fixed at create (tlpk_api.cpp: krylov_geometry).  The workgroup
// counts are the slot counts of the partial sums, so they fix the order of the additions.
struct KrylovGeom {
    i32 *long_rows = nullptr, *long_cols = nullptr; i64 n_long_rows = 0, n_long_cols = 0;
    int g_cols = 0, g_rows = 0;       // workgroups of the short columns (4 lanes each) and of the short rows (8 lanes each) of a 1024-thread gather kernel
    int g_lcols = 0, g_lrows = 0;     // workgroups that share the long columns / the long rows
    int g_vec = 0;                    // workgroups of the vector kernels (order m for conjugate gradients, n + m for MINRES and TriCG)
};
struct CgArrays {
    CgScalars *sc = nullptr;
    double *x = nullptr, *p = nullptr, *q = nullptr, *t = nullptr;
    double *Minv = nullptr;                       // Jacobi: 1 / diag(A D A' + Rd); nullptr = no preconditioner
    double *slots_r = nullptr, *slots_v = nullptr;   // partial sums of p'q (row kernel) and of r'z (vector kernels), one per workgroup, added in slot order by the consumer
    KrylovGeom geo;                               // k_cg_rows: g_rows (at least 1) + g_lrows workgroups; k_cg_cols and k_cg_jacobi size their own grids
};
void launch_cg_jacobi(hipStream_t st, const DevArrays &a, const CgArrays &c, const double *D, const double *regD);
// r (= a.ctx.xw) holds b: x = 0, p = M^-1 r, gamma, tolerance, outcome (a zero right-hand side is solved at once).
// c2 (here and below, for the three methods): not null = a PAIR of right-hand sides in the same launches.  Number 0 works on c's vectors and slots, number 1
// on c2's (conjugate gradients: its b / r in the second half of xw, at xw2), and c2->sc holds the TWO scalar blocks of the pair, contiguous; what c2 shares
// with c (the diagonals, the geometry) is read from c.  Each right-hand side stops on its own (krylov_reduce.hpp).
void launch_cg_init(hipStream_t st, const DevArrays &a, const CgArrays &c, double atol, double rtol, i64 itmax, const CgArrays *c2 = nullptr);
// iteration k (0-based) of the solve: four launches; returns their number
int launch_cg_iter(hipStream_t st, const DevArrays &a, const CgArrays &c, const double *D, const double *regD, i64 k, const CgArrays *c2 = nullptr);

// ---- matrix-free K2: MINRES on [-E A'; A Rd] [dx; dy] = [xi_d; xi_p] (krylov_k2_kernels.hip; DESIGN.md section 1b''''') ----
// The recurrence's state, kept twice: iteration k reads st[k & 1] and ONE thread of its last kernel writes st[(k + 1) & 1]
struct MrState { double beta, oldb, dbar, eps, cs, sn, phibar, pad; };
struct MrScalars {
    MrState st[2];
    double tol;           // atol + rtol beta1
    double resid0, resid; // beta1 = sqrt(b' M^-1 b) / phibar after the last completed iteration
    double alpha;         // of the running iteration: written by k_mr_step, read by k_mr_rot
    long long outcome;    // CG_RUNNING until a kernel decides, then (outcome code) | (deciding iteration, 1-based) << 8
    long long iters;      // completed iterations
    long long itmax;
    long long pad[9];
};
static_assert(sizeof(MrScalars) == 256, "MrScalars layout");
struct MrArrays {
    MrScalars *sc = nullptr;
    double *r[2] = {nullptr, nullptr};            // r1 / r2 of the Lanczos recurrence, rotating by parity; order N = n + m, stored [n-part; m-part] like every vector here
    double *z[2] = {nullptr, nullptr};            // M^-1 r[.]; without a preconditioner z[.] IS r[.] (the same storage)
    double *u = nullptr, *x = nullptr;
    double *w[2] = {nullptr, nullptr};
    double *Minv = nullptr;                       // Jacobi: 1 / diag(E_j, s_i); nullptr = no preconditioner
    double *slots_a = nullptr, *slots_g = nullptr;   // partial sums of v'u (k_mr_op) and of r'z (k_mr_init, k_mr_step), one per workgroup
    KrylovGeom geo;                               // k_mr_op: g_cols + g_rows + g_lcols + g_lrows workgroups, in this order
};
void launch_mr_diag(hipStream_t st, i64 n, const double *theta, const double *regP, double *E);
void launch_mr_jacobi(hipStream_t st, const DevArrays &a, const MrArrays &c, const double *E, const double *regD);
// b = [xi_d; xi_p]: x = w = 0, z = M^-1 b, beta1, tolerance, outcome (a zero right-hand side is solved at once); two launches.  xi_p, xi_d: one
// pointer, or the two of a pair (c2 not null)
void launch_mr_init(hipStream_t st, const DevArrays &a, const MrArrays &c, const double *const *xi_p, const double *const *xi_d, double atol, double rtol, i64 itmax,
                    const MrArrays *c2 = nullptr);
// iteration k (0-based) of the solve: three launches; returns their number
int launch_mr_iter(hipStream_t st, const DevArrays &a, const MrArrays &c, const double *E, const double *regD, i64 k, const MrArrays *c2 = nullptr);

// ---- matrix-free K2, quasi-definite form: TriCG on [Rd A; A' -E] [dy; dx] = [xi_p; xi_d] (krylov_sqd_kernels.hip; DESIGN.md section 1b'''''') ----
// The recurrence's state, kept twice like MrState: beta_k, gamma_k (the norms that scaled v_k, u_k), the inverse of the previous 2 x 2 pivot block
// D (symmetric) and the previous pi
struct TcState { double beta, gamma, i00, i01, i11, pi0, pi1, pad; };
struct TcScalars {
    TcState st[2];
    double tol;           // atol + rtol rho_0
    double resid0, resid; // rho_0 = hypot(beta1, gamma1) / rho_k after the last completed iteration
    double alpha;         // of the running iteration: written by k_tc_step, read by k_tc_upd
    long long outcome;    // as MrScalars: CG_RUNNING, then (outcome code) | (deciding iteration, 1-based) << 8
    long long iters;      // completed iterations
    long long itmax;
    long long pad[9];
};
static_assert(sizeof(TcScalars) == 256, "TcScalars layout");
struct TcArrays {
    TcScalars *sc = nullptr;
    long long *bad = nullptr;                     // update: the smallest node with a non-positive or non-finite diagonal entry, LLONG_MAX = none
    double *W = nullptr, *Winv = nullptr;         // the metric [E; Rd] and its reciprocal; order N = n + m, stored [n-part; m-part] like every vector here
    double *w[2] = {nullptr, nullptr};            // [u_k; v_k] and [u_{k-1}; v_{k-1}], rotating by parity
    double *t = nullptr, *x = nullptr;            // [p; q] of the iteration; the iterate [dx; dy]
    double *g[2] = {nullptr, nullptr};            // the two columns of G = [Gy; Gx], updated in place row by row
    double *slots_a = nullptr, *slots_g = nullptr, *slots_b = nullptr;   // partial sums of alpha (k_tc_op), of p'E^-1 p and of q'Rd^-1 q (k_tc_init, k_tc_step)
    KrylovGeom geo;                               // k_tc_op: g_cols + g_rows + g_lcols + g_lrows workgroups, in this order
};
// W, 1 / W and the quasi-definiteness check (one launch; *c.bad must hold LLONG_MAX before it)
void launch_tc_diag(hipStream_t st, const DevArrays &a, const TcArrays &c, const double *theta, const double *regP, const double *regD);
// b = [xi_d; xi_p]: beta1, gamma1, v_1, u_1, x = G = 0, tolerance, outcome (a zero right-hand side is solved at once); two launches
// xi_p, xi_d: one pointer, or the two of a pair (c2 not null)
void launch_tc_init(hipStream_t st, const DevArrays &a, const TcArrays &c, const double *const *xi_p, const double *const *xi_d, double atol, double rtol, i64 itmax,
                    const TcArrays *c2 = nullptr);
// iteration k (0-based) of the solve: three launches; returns their number
int launch_tc_iter(hipStream_t st, const DevArrays &a, const TcArrays &c, i64 k, const TcArrays *c2 = nullptr);

// new values on an analysed pattern (refresh_kernels.hip): w[t] = value(a[t]) * value(b[t]); out[q] = value(src[q]); the strided copy of a dense A
void launch_refresh_pairs(hipStream_t st, i64 np, const i32 *a, const i32 *b, const double *nz, double *w);
void launch_refresh_gather(hipStream_t st, i64 n, const i32 *src, const double *nz, double *out);
void launch_refresh_dense(hipStream_t st, i64 m, i64 n, const double *A, i64 lda, double *dA, i64 dlda);
// ... for the selected LPs of a stack (tlpk_ipm_batch_refill): lp_of[p] = the LP that owns entry p of nz, flag[k * stride] != 0 selects LP k; an element whose
// LP is not selected is left alone
void launch_refresh_pairs_sel(hipStream_t st, i64 np, const i32 *a, const i32 *b, const double *nz, double *w, const i32 *lp_of, const double *flag, int stride);
void launch_refresh_gather_sel(hipStream_t st, i64 n, const i32 *src, const double *nz, double *out, const i32 *lp_of, const double *flag, int stride);

}  // namespace tlpk
