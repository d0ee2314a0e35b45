/*
 * tlpk.h -- C ABI of libtlpk.so: the MI355X (gfx950) backend for Tulip's normal-equations
 * Newton step.  This is the drop-in boundary: a Julia `HIPNormalEquations <: AbstractKKTSolver`
 * (tulip.jl_amd/julia/hip.jl) binds these entry points with `ccall`.
 *
 * Reference interface replaced (citations into /root/reference):
 *   tlpk_create   <-> KKT.setup(A, ::K1, backend)            src/KKT/KKT.jl:59, Cholmod/spd.jl:5-20
 *   tlpk_update   <-> KKT.update!(kkt, θinv, regP, regD)      src/KKT/KKT.jl:65-83, Cholmod/spd.jl:22-50
 *   tlpk_solve    <-> KKT.solve!(dx, dy, kkt, ξp, ξd)         src/KKT/KKT.jl:85-100, Cholmod/spd.jl:52-70
 *   tlpk_backend_name / tlpk_system_name <-> KKT.backend / KKT.linear_system   KKT.jl:107-121
 *   tlpk_destroy  <-> GC finalizer of the solver object
 *
 * Conventions: plain pointers and sizes only; every function returns a TLPK_* code and never
 * throws, aborts or retains a host pointer after it returns.  Host-pointer entry points block
 * until results are in host memory.  One handle is used by one thread at a time; several
 * handles may coexist.  Numeric factorise + solves run on the device; the analyse phase
 * (ordering, elimination tree, supernodes, schedules) runs on the host inside tlpk_create.
 */
#ifndef TLPK_H
#define TLPK_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tlpk_handle tlpk_handle;

/* return codes */
#define TLPK_OK 0
#define TLPK_NOT_POSDEF 1   /* -> PosDefException in the glue (spd.jl:47); handle stays usable */
#define TLPK_BADARG 2       /* -> DimensionMismatch / ArgumentError (spd.jl:26-34) */
#define TLPK_OOM 3          /* -> OutOfMemoryError (HSD.jl:327-329) */
#define TLPK_HIPERR 4       /* HIP runtime error; tlpk_last_error() has the text */
#define TLPK_NO_DEVICE 5    /* numeric call on an analyse-only handle, or no GPU visible */
#define TLPK_TOO_LARGE 6    /* symbolic nnz(L) exceeds the memory budget (SURVEY.md App. C gate) */
#define TLPK_NOT_FACTORED 7 /* solve before a successful update */
#define TLPK_INTERNAL 8

/* linear system (KKT.jl:37-56 / systems.jl) */
#define TLPK_SYSTEM_K1 0     /* normal equations  A D A' + Rd, Cholesky            (Cholmod/spd.jl) */
#define TLPK_SYSTEM_K2 1     /* augmented system [-(Theta^-1+Rp) A'; A Rd], signed Cholesky L S L' = the LDL' of a
                                quasi-definite matrix without pivoting (Cholmod/sqd.jl, LDLFactorizations/ldlfact.jl);
                                row_block gives per-block ordering, stream groups and a root front; sharded / multi-device handles
                                replicate the root front (pivots of both signs), its assembled entries come from rank 0 */

/* tlpk_options.krylov */
#define TLPK_KRYLOV_NONE 0
#define TLPK_KRYLOV_CG 1        /* K1: conjugate gradients on the normal equations */
#define TLPK_KRYLOV_MINRES 16   /* K2: MINRES on the augmented system.  The K2 methods start at 16; 2 - 15 and every other value: TLPK_BADARG */
#define TLPK_KRYLOV_TRICG 32    /* K2 in its symmetric quasi-definite form [Rd A; A' -E]: TriCG.  The quasi-definite K2 methods start at 32; 33 is reserved for
                                   TriMR (the minimum-residual sibling, not implemented) and refused like any unknown value */
#define TLPK_PRECOND_NONE 0
#define TLPK_PRECOND_JACOBI 1

/* ordering selector */
#define TLPK_ORDER_AMD 0
#define TLPK_ORDER_NATURAL 1
#define TLPK_ORDER_USER 2

typedef struct tlpk_options {
    int32_t struct_size;       /* = sizeof(tlpk_options); set by tlpk_default_options */
    int32_t device;            /* HIP device ordinal; -1 = analyse only (no device is touched) */
    int32_t ordering;          /* TLPK_ORDER_* */
    int32_t relax;             /* supernode amalgamation: 0 = fundamental only, 1 = relaxed */
    int32_t profile;           /* 1 = time every kernel class with HIP events (tlpk_kernel_times) */
    int32_t rank, nranks;      /* block-angular sharding over ranks (nranks = 1: everything local) */
    int32_t streams;           /* concurrent stream groups for block-angular LPs: 0 = auto (2), 1 = single group; each group also owns a side stream */
    const int64_t *user_perm;  /* TLPK_ORDER_USER: perm[new] = old, in index_base, length m; system = K2: length m + n, old < n is variable
                                * node old, old = n + i is constraint node i.  Not with row_block, not on tlpk_create_multi handles */
    const int64_t *row_block;  /* block-angular hook (length m): block id >= 0, or -1 for a linking
                                  row; NULL = general sparse.  Blocks are ordered independently,
                                  linking rows last as one dense root supernode. */
    int64_t mem_budget_bytes;  /* 0 = 90 % of the device's free memory (or unlimited if device=-1) */
    int32_t system;            /* TLPK_SYSTEM_K1 (default) | TLPK_SYSTEM_K2 */
    int32_t refine_steps;      /* iterative-refinement steps per solve on the residuals of the augmented system (each step = one more
                                  pair of sweeps); 0 = none = the reference's behaviour (spd.jl:68 leaves it as a TODO).  K1; one rank or a
                                  tlpk_create_multi handle (sharded handles: tlpk_refine_local / tlpk_refine_finish, the caller owns the collective) */
    int32_t detect_blocks;     /* 1 (and row_block == NULL): find the block-angular structure of THIS matrix with tlpk_detect_blocks --
                                  the hook that survives Tulip's presolve, which renumbers the rows before KKT.setup sees them
                                  (model.jl:88-131).  No structure found: general sparse path (tlpk_create) / TLPK_BADARG (tlpk_create_multi) */
    int32_t keep_on_too_large; /* 1: tlpk_create returns a LIVE analyse-only handle together with TLPK_TOO_LARGE (tlpk_info / tlpk_last_error then describe what did not
                                  fit; the caller must destroy it).  0 (default): no handle on any failure -- the message is in tlpk_last_create_error() */
    int64_t max_link_rows;     /* detect_blocks: most linking rows to accept; 0 = max(64, m / 20) */
    /* Dense (linking) columns, K1 only.  A column of A with c entries puts a c x c clique into A*D*A'.  With dense_cols = 1 the
     * columns that qualify stay out of A*D*A' and become k extra nodes of a partially augmented, symmetric quasi-definite system
     *     [ A_s D_s A_s' + Rd    A_d            ] [ dy   ]   [ xi_p + A_s D_s xi_d_s ]
     *     [ A_d'                 -(Theta_d^-1 + Rp_d) ] [ dx_d ] = [ xi_d_d                ]
     * of order m + k, factorised by the signed Cholesky of K2 (the k nodes last / in the root front); dx_s = D_s (A_s' dy - xi_d_s).
     * The caller still solves K1: same vectors, same results (up to rounding), refinement allowed.  Refused with K2, nranks > 1 and
     * tlpk_create_multi (TLPK_BADARG). */
    int32_t dense_cols;        /* 0 = off (default): every column is formed into A*D*A'; 1 = qualifying columns become augmented nodes */
    int32_t max_dense_cols;    /* cap on k; 0 = 1024.  More qualifying columns: the densest are taken (ties: lower index), the rest stay in A*D*A' */
    int64_t dense_col_min;     /* a column with MORE than this many entries qualifies; 0 = 1000 */
    const int64_t *col_dense;  /* optional, length n: nonzero = this column qualifies whatever its count (e.g. first-stage variables);
                                  like row_block, only meaningful on the matrix the caller analyses (no presolve in between) */
    /* Matrix-free handle (the reference's Krylov family, src/KKT/Krylov/spd.jl): no analysis, no factor, O(nnz(A) + m + n) device memory.  See tlpk_create. */
    int32_t krylov;            /* TLPK_KRYLOV_NONE 0 (default: analyse + factorise) | TLPK_KRYLOV_CG 1: K1, conjugate gradients on
                                  (A D A' + Rd) dy = xi_p + A D xi_d, matrix-free (src/KKT/Krylov/spd.jl) | TLPK_KRYLOV_MINRES 16: K2 (system must be
                                  TLPK_SYSTEM_K2), MINRES on [-E A'; A Rd] [dx; dy] = [xi_d; xi_p], E = theta^-1 + Rp (src/KKT/Krylov/sid.jl) |
                                  TLPK_KRYLOV_TRICG 32: K2, TriCG on the quasi-definite form [Rd A; A' -E] [dy; dx] = [xi_p; xi_d] (src/KKT/Krylov/sqd.jl) */
    int32_t krylov_precond;    /* 0 = none (the reference) | 1 = Jacobi, rebuilt by every update: CG: M = diag(A D A' + Rd); MINRES: the positive
                                  definite block diagonal M = diag(E_j, sum_{E_j > 0} A_ij^2 / E_j + Rd_i); TriCG: must be 0 (E and Rd are its inner products) */
    int64_t krylov_itmax;      /* 0 = twice the order of the system (Krylov.jl's default): 2 m for CG, 2 (m + n) for MINRES; TriCG: 2 (m + n) by this
                                  library's convention -- Krylov.jl's own default for tricg could not be read when this was written */
    double  krylov_atol, krylov_rtol;   /* 0 = sqrt(eps) (spd.jl:66-67); < 0 or non-finite: TLPK_BADARG */
} tlpk_options;

typedef struct tlpk_stats {
    int64_t m, n, nnzA;
    int64_t nnzS;              /* lower triangle of A*D*A' + Rd, incl. diagonal (dense_cols: of the order-(m + k) matrix) */
    int64_t nnzL;              /* nnz of the Cholesky factor (incl. diagonal) */
    int64_t nnzL_stored;       /* doubles stored in supernodal panels (>= nnzL) */
    double  flops_chol;        /* sum_j l_j^2 (CHOLMOD `fl` convention) */
    double  flops_panel;       /* flops executed by the dense panel kernels (incl. padding zeros) */
    int64_t n_supernodes;
    int64_t n_levels;          /* depth of the supernodal elimination tree */
    int64_t max_front;         /* largest front order */
    int64_t n_pairs;           /* products in the A*D*A' assembly lists */
    int64_t device_bytes;      /* device memory held by this handle */
    int64_t launches_update, launches_solve;
    int64_t fail_col;          /* permuted column of the first non-positive pivot, or -1 */
    double  ms_analyse;        /* host analyse time */
    double  ms_last_update;    /* device time of the last update (HIP events, handle stream) */
    double  ms_last_solve;     /* device time of the last solve */
    int32_t n_local_blocks, n_blocks;
    int64_t root_panel_len;    /* doubles in the root (linking) panel reduced across ranks */
    double  flops_update;      /* flops EXECUTED by the fp64-MFMA update kernel per factorisation on the amalgamated
                                  (zero-padded) structure: 2*K*(lower-triangle target entries), summed over its launches */
    double  flops_update_alg;  /* ALGORITHMIC flops of that kernel: the share of flops_chol = sum_j l_j^2 whose target
                                  column lies outside column j's own 256-wide block column, sum_j (l_j - r_j)^2 with the
                                  true column counts l_j (no amalgamation zeros); <= flops_chol, <= flops_update */
    double  ms_enqueue_update; /* multi-device handles: host time from the entry of the last tlpk_update until the work of EVERY shard
                                  (root fronts included) was enqueued; ms_last_update is then the wall time of the whole call */
    int64_t refine_rejected;   /* refine_steps > 0: refinement steps of the last completed solve that did NOT shrink |r1|inf, or lifted |r2|inf beyond 16 x its
                                  value after the unrefined solve, and were discarded (a rejected step ends the refinement of that solve's RESULT; on one device the remaining steps are still enqueued -- solve, candidate, residuals, norms: the
                                  verdict is taken on the device without a host round trip -- and only their commit is skipped: a rejected step does not make the call cheaper); valid after tlpk_sync / a blocking solve */
    double  flops_update_chain;     /* round 6: the share of flops_update / flops_update_alg whose tiles run as items of the dependency-driven launches */
    double  flops_update_alg_chain; /* (k_chain: fronts with more than one block column on levels with few such fronts) instead of in k_update launches */
    int64_t chain_launches, chain_items;   /* number of those launches per factorisation and the items (update tiles, diagonal blocks, solve strips, reductions) they hold */
    int64_t n_dense_cols;      /* k: columns of A handled as augmented nodes (tlpk_options.dense_cols); tlpk_symbolic_get(h, "dense_cols") lists them.
                                  m, n, nnzA are the caller's; nnzS, nnzL, n_pairs, fail_col, ... describe the factored matrix of order m + k */
    double  flops_syrk;        /* dense-matrix handles (tlpk_create_dense): n m (m + 1), the flops of the lower triangle of A*D*A' on the matrix cores
                                  (2 per product); 0 on sparse handles */
    /* matrix-free handles (tlpk_options.krylov); 0 on every other handle.  (Placed in front of the tlpk_set_values pair, which stays the tail of the struct;
       tlpk_stats carries no size field, so any new field means a rebuild of the callers wherever it goes.) */
    int64_t krylov_iters;        /* CG / MINRES / TriCG iterations of the last solve (after tlpk_solve2_device: of its second right-hand side, like the next three) */
    int64_t krylov_iters_total;  /* since the last update */
    int64_t krylov_converged;    /* 1 = the last solve met the stopping rule; 0 = it stopped at itmax or broke down */
    double  krylov_resid0, krylov_resid;   /* sqrt(r' M^-1 r) at x = 0 and at exit of the last solve (MINRES: beta1 and phibar, the recurrence's value of it; TriCG: rho_0 and rho_k, the
                                  residual in the norm of diag(Rd, E)^-1) */
                                 /* tlpk_symbolic_get(h, "krylov_unsolved"): one entry, the number of solves since create that did NOT meet the stopping
                                    rule (what a loop of many solves checks once at its end instead of reading krylov_converged after every solve) */
    double  ms_last_set_values; /* device time of the last tlpk_set_values* (HIP events on the handle's stream; multi-device handles: the slowest shard);
                                   host time on analyse-only handles */
    int64_t set_values_bytes;  /* device memory held by the maps of tlpk_set_values (part of device_bytes); 0 before the first call */
} tlpk_stats;

/* per-kernel-class timing, filled when options.profile = 1 */
#define TLPK_KC_ASSEMBLE 0
#define TLPK_KC_EXTEND_ADD 1
#define TLPK_KC_POTRF 2
#define TLPK_KC_TRSM 3
#define TLPK_KC_UPDATE 4     /* fp64-MFMA panel update (the dominant kernel) */
#define TLPK_KC_SOLVE_FWD 5
#define TLPK_KC_SOLVE_BWD 6
#define TLPK_KC_SPMV 7
#define TLPK_KC_UPDATE_REDUCE 8   /* split-K: ordered sum of partial tiles + application to the targets */
#define TLPK_KC_CHAIN 9           /* round 6: dependency-driven launches (k_chain): update tiles + diagonal blocks + triangular solves of a level's multi-block-column fronts */
#define TLPK_KC_COUNT 10
typedef struct tlpk_kernel_times {
    double  ms[TLPK_KC_COUNT];       /* summed duration of the class in the last update+solve */
    int64_t launches[TLPK_KC_COUNT];
} tlpk_kernel_times;

void tlpk_default_options(tlpk_options *opt);

/* A is m x n CSC with int64 indices (Julia SparseMatrixCSC{Float64,Int}); index_base in {0,1}.
 * A is copied; nothing is retained.  Runs the whole analyse phase and uploads the symbolic
 * structures.  Does NOT perform the throw-away numeric factorisation of spd.jl:14-17.
 * Return value != TLPK_OK: *out = NULL and tlpk_last_create_error() holds the diagnostic (for TLPK_TOO_LARGE: the bytes needed against the
 * budget, and -- K1 with a dense column of A -- the hint that KKT_System = K2 does not form A*D*A', or that K1 with dense_cols = 1 does not either).  Only with opt->keep_on_too_large = 1 does
 * TLPK_TOO_LARGE return a live analyse-only handle (tlpk_info: symbolic nnz(L) ...), which the caller destroys. */
int tlpk_create(tlpk_handle **out, int64_t m, int64_t n, const int64_t *colptr,
                const int64_t *rowval, const double *nzval, int index_base,
                const tlpk_options *opt);
/* Matrix-free handle: opt->krylov = TLPK_KRYLOV_CG (K1; the reference's src/KKT/Krylov/spd.jl).  tlpk_create then skips ordering, the pattern of S,
 * supernodes, lists and schedules and keeps only the CSC and the row-wise copy of A in the caller's order: tlpk_stats nnzS = nnzL = nnzL_stored = n_pairs =
 * n_supernodes = 0, flops_* = 0, tlpk_get_perm = the identity, every symbolic array empty, tlpk_get_factor: TLPK_BADARG.  The memory gate counts the copies of A
 * and the vectors.  TLPK_BADARG (sentence in tlpk_last_create_error()): system = K2 (TLPK_KRYLOV_CG), nranks > 1, dense_cols, refine_steps > 0, user_perm, an unknown krylov /
 * krylov_precond value, krylov_itmax < 0, a negative or non-finite tolerance; tlpk_create_multi and tlpk_create_dense refuse the option.  row_block,
 * detect_blocks, ordering, relax and streams are ignored.  device = -1: an analyse-only handle (numeric calls: TLPK_NO_DEVICE).  The split-phase calls
 * (tlpk_*_local / tlpk_*_finish, tlpk_root_*, tlpk_refine_*) do not apply: TLPK_BADARG.
 *   update : D = 1 / (theta^-1 + Rp), Rd is kept; Jacobi: M_i = sum_j A_ij^2 D_j + Rd_i in one pass over the rows (an empty row with Rd_i = 0 has
 *            M_i = 0 and is left unscaled, M^-1_i = 1).  Never TLPK_NOT_POSDEF.
 *            tlpk_update_device_async is the blocking call.
 *   solve  : b = xi_p + A (D .* xi_d); conjugate gradients from x = 0 with z = M^-1 r, gamma = r'z: SOLVED when sqrt(gamma) <= atol + rtol sqrt(gamma at x = 0)
 *            (a zero right-hand side: in 0 iterations), NOT solved after krylov_itmax iterations, or when p'Sp <= 0 or a scalar is not finite (Krylov.jl's cg);
 *            then dy = x, dx = D .* (A' dy - xi_d).  A solve that is NOT solved still writes its last iterate and returns TLPK_OK, as the reference does
 *            (spd.jl:100-101 does not look at the outcome): tlpk_stats.krylov_converged / krylov_iters / krylov_resid say what happened -- a caller that
 *            needs a solved system must read them.  The number of launches depends on the data, so tlpk_solve_device on such a handle BLOCKS until the outcome
 *            is known (iterations are enqueued in chunks, the host reads the outcome word between chunks); dx / dy are complete after tlpk_sync as usual.
 *            Two solves of the same data are bit-identical (no atomics, ordered reductions).
 *   pair   : tlpk_solve2_device runs BOTH right-hand sides through one sequence of launches (all three methods, with and without Jacobi): one pass over A per
 *            iteration, one set of launches and one host round trip per chunk for the two systems.  Each right-hand side has its own scalar block,
 *            tolerance, outcome and counters and stops on its own; one that is solved, broken down or at itmax is parked (nothing of it is read or
 *            written any more) while the launches go on for the other.  dx, dy, iterations, outcome, resid0 and resid of each one are bit for bit those
 *            of tlpk_solve_device on it alone.  The statistics read as after the two solves one behind the other: krylov_iters / krylov_converged /
 *            krylov_resid0 / krylov_resid describe the SECOND right-hand side, krylov_iters_total grows by both counts, "krylov_unsolved" by the number
 *            that did not meet the rule; launches_solve is that of the pair, 5 + 4 per round (CG; 3 per round when n = 0) or 2 + 3 per round (MINRES, TriCG),
 *            which is the count of the single solve of the longer one.  What the pair itself did:
 *              tlpk_symbolic_get(h, "krylov_pair")           7 entries: paired solves since create, pairs that fell back to two solves since create; of the last
 *                                                            pair the iterations of number 0 and 1, their outcome codes (1 solved, 2 itmax, 3 breakdown), the
 *                                                            rounds of launches enqueued
 *              tlpk_symbolic_get_f64(h, "krylov_pair_resid") 4 entries: resid0, resid of number 0, then of number 1
 *            (zeros before the first pair and on every other handle).  The second set of vectors (CG: 3 of order m and 1 of order n; MINRES: 6 of order
 *            n + m, 8 with Jacobi; TriCG: 6) is allocated by the FIRST pair, not at create: mem_budget_bytes and the footprint of a handle that never
 *            pairs are unchanged.  If that allocation fails or would cross mem_budget_bytes, every pair runs as two solves (counted above).
 *            TLPK_KRYLOV_PAIR=0 in the environment at create keeps the two solves.  Device pointers only; the buffers follow the rule stated at
 *            tlpk_solve2_device.
 *   tlpk_set_values* refreshes the copies of A; the device-resident loops (tlpk_ipm_*, tlpk_mpc_*) run through the same solve path.
 * opt->krylov = TLPK_KRYLOV_MINRES with opt->system = TLPK_SYSTEM_K2 (the reference's src/KKT/Krylov/sid.jl) is the same handle -- the same analysis, refusals,
 * identity permutation (of the n + m nodes of K2: tlpk_get_perm writes n + m entries, as on a direct K2 handle), tlpk_set_values*, loops, blocking solve, chunked enqueue and stats fields -- with preconditioned MINRES (Paige & Saunders) on the
 * augmented system of order n + m.  system = K1 with it, and TLPK_KRYLOV_CG with K2, are TLPK_BADARG.  tlpk_linear_system: "Augmented system (K2)".
 *   update : E = theta^-1 + Rp and Rd are kept; 1 / E is never formed outside the preconditioner, so columns with E_j = 0 (free variables without
 *            regularisation) and Rd = 0 are fine as long as K is nonsingular.  Jacobi: M = diag(E_j, s_i), s_i = sum_{j: E_j > 0} A_ij^2 / E_j + Rd_i, in one pass
 *            over the rows; an entry of M that is 0 is replaced by 1.  Never TLPK_NOT_POSDEF.
 *   solve  : K [dx; dy] = [xi_d; xi_p], K = [-E A'; A Rd] (KKT.jl:70-75), from x = 0.  Lanczos with z = M^-1 r, beta = sqrt(r'z), one Givens rotation per step;
 *            phibar is the recurrence's sqrt(r' M^-1 r).  SOLVED when phibar <= atol + rtol beta1 (a zero right-hand side: in 0 iterations); NOT solved after
 *            krylov_itmax iterations (0 = 2 (m + n)), when r'z < 0 or a scalar is not finite, or when beta = 0 (the Krylov space is exhausted) with phibar
 *            still above the tolerance.  This is the only stopping rule: Krylov.jl's minres may have others (a test on ||A r||, a condition-number limit) that
 *            could not be compared.  As above, a solve that is NOT solved writes its last iterate and returns TLPK_OK (sid.jl:100-104).
 *            launches_solve = 2 + 3 per enqueued iteration.
 * opt->krylov = TLPK_KRYLOV_TRICG with opt->system = TLPK_SYSTEM_K2 (the reference's src/KKT/Krylov/sqd.jl, Krylov.jl's tricg) is again the same handle -- analysis,
 * refusals, identity permutation of the n + m nodes, tlpk_set_values*, loops, blocking solve, chunked enqueue, stats fields, "Augmented system (K2)" -- with
 * TriCG (Montoison & Orban) on the symmetric quasi-definite form [Rd A; A' -E] [dy; dx] = [xi_p; xi_d], called with M = Rd^-1, N = E^-1 (sqd.jl:74-77, 87-92).
 * system = K1 with it is TLPK_BADARG, and so is krylov_precond != 0: the two diagonal blocks are the method's inner products, there is nothing left to
 * precondition with.  33 (TriMR) is reserved and refused.  Device memory (the gate): 36 nnz + 136 n + 168 m + 65536 bytes -- the copies of A and the vectors of
 * every handle (36 nnz + 72 n + 104 m) and eight vectors of order n + m ([E; Rd], its reciprocal, [u; v] twice, [p; q], [dx; dy], the two columns of G).
 *   update : E = theta^-1 + Rp, Rd and their reciprocals are kept (one launch: launches_update = 1).  The method needs E_j > 0 and Rd_i > 0; the reference
 *            forms inv(0) silently, this library does not: the kernel records the smallest node with a non-positive or non-finite entry, numbered as a K2
 *            handle numbers its nodes (j for E_j, n + i for Rd_i), and the update returns TLPK_NOT_POSDEF with tlpk_stats.fail_col = that node and
 *            tlpk_last_error "... not quasi-definite ...".  The handle stays usable and NOT factored (a solve: TLPK_NOT_FACTORED) until an update succeeds --
 *            the code an interior-point loop answers by raising its regularisation (HSD/step.jl:35-51).
 *   solve  : v_k in R^m, u_k in R^n with <v, v> = v'Rd v, <u, u> = u'E u tridiagonalise A by two short recurrences (Saunders, Simon & Yip); the Galerkin
 *            iterate comes from the 2 x 2 block L D L' of the permuted projected matrix (diagonal blocks [1 alpha_k; alpha_k -1], sub-diagonal blocks
 *            [0 beta_k; gamma_k 0]); Krylov.jl factorises the same matrix scalar by scalar, the iterates agree in exact arithmetic.
 *            rho_k = hypot(beta_{k+1} pi_k[1], gamma_{k+1} pi_k[0]) = sqrt(r_p'Rd^-1 r_p + r_d'E^-1 r_d) of the residual; rho_0 = hypot(beta_1, gamma_1).
 *            SOLVED when rho_k <= atol + rtol rho_0 (a zero right-hand side: in 0 iterations); NOT solved after krylov_itmax iterations (0 = 2 (m + n)),
 *            when a scalar is not finite, or when a 2 x 2 pivot block loses its signature (det D_k >= 0: impossible in exact arithmetic).  A zero
 *            beta_{k+1} or gamma_{k+1} gives a zero Lanczos vector and the run goes on.  krylov_resid0 = rho_0, krylov_resid = rho_k.  As above, a solve that
 *            is NOT solved writes its last iterate and returns TLPK_OK (sqd.jl:94-96).
 *            launches_solve = 2 + 3 per enqueued iteration.
 * What to expect: conjugate gradients without a preconditioner (the reference: spd.jl:26 "TODO: preconditioner") or with Jacobi solve the early, well-conditioned
 * systems of an interior-point run in tens of iterations and stall on the late ones (DESIGN.md section 1b has the measured limits). */
/* Dense constraint matrix (the reference's dense backend, src/KKT/Dense/lapack.jl; K1 only).  A: m x n, column-major, leading dimension
 * lda >= m (a Julia Matrix{Float64}); copied, nothing retained.  The handle then behaves like any single-device K1 handle: natural order,
 * ONE dense front of m columns, A*D*A' + Rd formed on the fp64 matrix cores (timed as TLPK_KC_ASSEMBLE) straight into the front's panel,
 * the blocked dense Cholesky and the sweeps of the sparse handles, two dense matrix-vector products per solve (TLPK_KC_SPMV).  No pattern
 * of S and no assembly lists are built: host memory beyond the copy of A is O(m + schedule), tlpk_stats.n_pairs = 0.
 * Honoured options: device (-1 = analyse only), profile, mem_budget_bytes, keep_on_too_large; ordering, relax, streams are ignored.
 * TLPK_BADARG (sentence in tlpk_last_create_error()): A == NULL, lda < m, m < 1, system = K2, nranks > 1, row_block / detect_blocks,
 * user_perm, dense_cols, refine_steps > 0.  TLPK_TOO_LARGE: the device copy of A + the panel + workspace exceed the budget (the message
 * states the bytes).  The split-phase calls (tlpk_*_local / tlpk_*_finish, tlpk_root_*, tlpk_refine_*) do not apply: TLPK_BADARG. */
int tlpk_create_dense(tlpk_handle **out, int64_t m, int64_t n, const double *A, int64_t lda, const tlpk_options *opt);
void tlpk_destroy(tlpk_handle *h);

/* New numerical values on the analysed pattern: "analyse once, factorise many value sets" (branch-and-bound nodes, scenario re-solves, successive LPs,
 * re-scaling).  nzval: the values of the matrix given to tlpk_create / tlpk_create_multi in the caller's CSC order, len == nnzA; explicit zeros are values.
 * Nothing of the analysis is repeated and no array is reallocated: the products of the assembly lists and the value arrays of the copies of A are
 * recomputed in place, on the device, from maps that the FIRST call builds (one walk of the lists on the host) and uploads -- tlpk_stats.device_bytes grows
 * once by tlpk_stats.set_values_bytes.  The refreshed handle equals a fresh handle on the new values bit for bit.
 * After TLPK_OK the handle is analysed but NOT factored (solves: TLPK_NOT_FACTORED until the next successful update); a pending asynchronous update, pair or
 * refinement is completed / dropped as an update does.  TLPK_BADARG (NULL, len != nnzA, lda < m, a sparse call on a dense-matrix handle or the reverse)
 * leaves the handle untouched and factored; tlpk_last_error has the sentence.  Every handle kind: K1, K2, dense_cols, refine_steps, sharded (every rank passes
 * the full nzval), tlpk_create_multi (one call serves every shard), analyse-only (the host arrays are refreshed: tlpk_symbolic_get_f64(h, "pair_w")).
 * The _device variants take a pointer on the handle's device and enqueue on tlpk_stream(h): the caller orders its producer before that stream and may reuse
 * the buffer after tlpk_sync; single-device handles only (multi-device: TLPK_BADARG, analyse-only: TLPK_NO_DEVICE).
 * A handle with device-resident loops (tlpk_ipm_load): every tlpk_ipm_* / tlpk_mpc_* call except tlpk_ipm_reload and tlpk_ipm_get then returns TLPK_BADARG
 * until tlpk_ipm_reload has run. */
int tlpk_set_values(tlpk_handle *h, const double *nzval, int64_t len);                 /* host pointer; blocks */
int tlpk_set_values_device(tlpk_handle *h, const double *d_nzval, int64_t len);        /* device pointer; enqueued on tlpk_stream(h) */
/* Dense-matrix handles (tlpk_create_dense): column-major m x n, lda >= m. */
int tlpk_set_values_dense(tlpk_handle *h, const double *A, int64_t lda);
int tlpk_set_values_dense_device(tlpk_handle *h, const double *d_A, int64_t lda);

/* Host-pointer entry points (what the Julia glue calls). */
int tlpk_update(tlpk_handle *h, const double *theta_inv /*n*/, const double *regP /*n*/,
                const double *regD /*m*/);
int tlpk_solve(tlpk_handle *h, double *dx /*n*/, double *dy /*m*/, const double *xi_p /*m*/,
               const double *xi_d /*n*/);

/* Device-pointer entry points: same semantics, arguments are device pointers on the handle's
 * device, work is enqueued on the handle's stream; tlpk_sync waits and returns the status
 * (TLPK_NOT_POSDEF is reported by tlpk_update_device itself: it reads back one status word). */
int tlpk_update_device(tlpk_handle *h, const double *d_theta_inv, const double *d_regP,
                       const double *d_regD);
int tlpk_solve_device(tlpk_handle *h, double *d_dx, double *d_dy, const double *d_xi_p,
                      const double *d_xi_d);
/* tlpk_update_device without the wait for its status word.  Everything is enqueued; on block-angular handles the root (linking) front --
 * a dense front of a few hundred columns whose factorisation is a serial chain of diagonal blocks, ~1.5 ms with the chip nearly idle --
 * goes to a stream of its own, so that the block-level forward sweeps of the next solve overlap it.  The verdict arrives with the next
 * tlpk_sync (TLPK_NOT_POSDEF; the handle stays usable); solves enqueued in between are speculative.  Unsharded handles; falls back to the
 * blocking call where there is nothing to overlap (no root front, profile mode, graph replay).  MEASURED SLOWER than the blocking call on
 * the bench workloads (C4 +1.1 ms, north-star instance +1.9 ms per step: the root front's ~20 dependent small launches queue behind the
 * chip-filling sweep workgroups; profiles/r03_async_update.txt) -- kept as an option, not used by default. */
int tlpk_update_device_async(tlpk_handle *h, const double *d_theta_inv, const double *d_regP, const double *d_regD);
/* Two right-hand sides in one pass over the factor (the solve sweeps are HBM-bound on the bytes of L: the pair costs little more than
 * one solve).  Same semantics and bit-identical results as two tlpk_solve_device calls.  Single-rank handles.  Tulip's HSD iteration
 * has such a pair: the h-system and the predictor (HSD/step.jl:63,79); tlpk_ipm_hsolve_newton uses it.  On a matrix-free handle
 * (tlpk_options.krylov) the pair is one sequence of launches for both iterations (see "pair" there).
 * Buffers: the four outputs are distinct from each other and from every input; the inputs may alias each other (the same right-hand
 * side may be given twice). */
int tlpk_solve2_device(tlpk_handle *h, double *d_dx0, double *d_dy0, const double *d_xi_p0, const double *d_xi_d0,
                       double *d_dx1, double *d_dy1, const double *d_xi_p1, const double *d_xi_d1);
int tlpk_sync(tlpk_handle *h);
void *tlpk_stream(tlpk_handle *h);           /* hipStream_t the kernels are launched on */

/* Block-angular sharding (nranks > 1): split-phase calls so that the caller owns the
 * collective (RCCL all-reduce over xGMI through whatever communicator it has).
 *   update : tlpk_update_local -> allreduce(sum) of tlpk_root_panel -> tlpk_update_finish
 *   solve  : tlpk_solve_local  -> allreduce(sum) of tlpk_root_rhs   -> tlpk_solve_finish
 * With nranks = 1 the split calls compose to exactly tlpk_update_device / tlpk_solve_device. */
int tlpk_update_local(tlpk_handle *h, const double *d_theta_inv, const double *d_regP,
                      const double *d_regD);
int tlpk_root_panel(tlpk_handle *h, double **d_ptr, int64_t *count);
int tlpk_update_finish(tlpk_handle *h);
int tlpk_solve_local(tlpk_handle *h, const double *d_xi_p, const double *d_xi_d);
int tlpk_root_rhs(tlpk_handle *h, double **d_ptr, int64_t *count);
int tlpk_solve_finish(tlpk_handle *h, double *d_dx, double *d_dy, const double *d_xi_d);
/* The pair of tlpk_solve2_device in split-phase form (two right-hand sides, one pass over this rank's part of the factor):
 *   tlpk_solve2_local -> allreduce(sum) of tlpk_root_rhs AND of tlpk_root_rhs2 -> tlpk_solve2_finish
 * (the two root right-hand sides are separate buffers of tlpk_root_rhs's length).  Bit-identical to two split solves. */
int tlpk_solve2_local(tlpk_handle *h, const double *d_xi_p0, const double *d_xi_d0, const double *d_xi_p1, const double *d_xi_d1);
int tlpk_root_rhs2(tlpk_handle *h, double **d_ptr, int64_t *count);
int tlpk_solve2_finish(tlpk_handle *h, double *d_dx0, double *d_dy0, const double *d_xi_d0, double *d_dx1, double *d_dy1, const double *d_xi_d1);
/* Iterative refinement on a sharded handle (K1), one step = one more split solve on the residuals of the augmented system
 * (the equations of /root/reference/src/KKT/KKT.jl:70-75; the reference leaves refinement as a TODO, src/KKT/Cholmod/spd.jl:68):
 *   tlpk_refine_local(h, dx, dy, xi_p, xi_d) -> allreduce(sum) of tlpk_root_rhs -> tlpk_refine_finish(h, dx, dy)
 * after a finished solve, as often as wanted; dx / dy in the layout tlpk_solve_finish leaves (a rank's own columns and block rows,
 * the linking rows replicated) are corrected in place.  Every rank forms the residuals of the rows / columns it owns and its PARTIAL
 * sums of the linking rows; the reduction inside the solve completes them.  tlpk_options.refine_steps does this inside
 * tlpk_solve_device (one rank) and inside tlpk_solve of a tlpk_create_multi handle (the library owns the reductions there); on a
 * sharded handle the caller owns the collective, hence the split form.  With nranks = 1 the two calls compose to exactly one
 * refinement step of tlpk_solve_device. */
int tlpk_refine_local(tlpk_handle *h, const double *d_dx, const double *d_dy, const double *d_xi_p, const double *d_xi_d);
int tlpk_refine_finish(tlpk_handle *h, double *d_dx, double *d_dy);
/* Refinement on demand: K1 AND K2, chosen per solve, one system or a pair.  tlpk_polish_device takes any (dx, dy) -- normally the output of a finished
 * solve against the current factor -- and corrects it in place by up to `steps` guarded refinement steps on
 *   r1 = xi_p - A dx - Rd dy        r2 = xi_d + (theta_inv + Rp) dx - A' dy
 * with the theta_inv, Rp, Rd of the last update.  A step is one more solve with (r1, r2) as right-hand side; the candidate is kept only if |r1|inf shrinks
 * and |r2|inf stays within 16 x of its value at entry (the rule of tlpk_options.refine_steps), decided on the device; after the first rejected step the
 * remaining steps change nothing.  No host synchronisation: the work is enqueued on tlpk_stream(h) and complete after tlpk_sync.  steps = 0 measures
 * only: one pass over A, no sweep, dx and dy untouched.  On a K1 handle, tlpk_solve_device + tlpk_polish_device(steps = s) equals bit for bit the solve of
 * a handle created with refine_steps = s.
 * tlpk_polish2_device: two systems at once -- the residuals of both from ONE pass over A, each correction ONE paired pass over L (as tlpk_solve2_device),
 * every state word per system: each system's dx, dy and report are bit for bit those of tlpk_polish_device on it alone.  The four outputs are distinct from
 * each other and from every input; the inputs may alias each other.  tlpk_polish: host pointers, blocks.
 * Report (valid after tlpk_sync or a blocking call): tlpk_symbolic_get(h, "polish") = steps asked, accepted, rejected of system 0, then of system 1 (6 entries);
 * tlpk_symbolic_get_f64(h, "polish_resid") = per system |r1|inf, |r2|inf at entry and |r1|inf, |r2|inf of what was kept (8 entries);
 * tlpk_symbolic_get(h, "polish_bytes") = the device memory the first call allocated (part of device_bytes).  All zero before the first call and on every
 * other kind of handle; tlpk_stats.refine_rejected is not touched.
 * Handles: single-device handles with a factor -- K1 (row_block, dense_cols, refine_steps > 0 included) and K2.  Refused, in this order: a NULL handle;
 * a multi-device, sharded (nranks > 1), dense-matrix, matrix-free or batch-loaded handle; a NULL pointer; steps < 0; an unfinished split-phase solve, pair
 * or refinement step (all TLPK_BADARG, with a sentence in tlpk_last_error); TLPK_NO_DEVICE; TLPK_NOT_FACTORED.
 * Memory: the first call allocates the residuals and corrections (2 (m + n) doubles per system; the second system's by the first pair) and, on a K2 handle
 * (which holds the incidence matrix of the augmented system, not A), CSC and CSR copies of A -- or shares those of the device-resident loops if an LP is
 * loaded; tlpk_set_values* marks them stale and the next call refreshes them.  Nothing is allocated at create.  An allocation that would cross
 * mem_budget_bytes: TLPK_OOM, and the handle stays usable. */
int tlpk_polish_device(tlpk_handle *h, double *d_dx, double *d_dy, const double *d_xi_p, const double *d_xi_d, int steps);
int tlpk_polish2_device(tlpk_handle *h, double *d_dx0, double *d_dy0, const double *d_xi_p0, const double *d_xi_d0,
                        double *d_dx1, double *d_dy1, const double *d_xi_p1, const double *d_xi_d1, int steps);
int tlpk_polish(tlpk_handle *h, double *dx, double *dy, const double *xi_p, const double *xi_d, int steps);   /* host pointers, blocks */
/* Copy the root panel (which = 0), the root rhs (which = 1) or the second root rhs of a pair (which = 2) out of (dir = 0) / into (dir = 1) a
 * caller-owned device buffer, on the handle's stream -- for callers whose communicator wants to
 * own the memory it reduces (torch.distributed tensors). */
int tlpk_root_copy(tlpk_handle *h, int which, int dir, double *d_buf);

/* Single-process multi-GPU (block-angular LPs only): ONE handle, driven by one host thread, shards the diagonal
 * blocks over `ngpus` devices of this node -- what a Julia process needs (`TlpHIP.Backend(row_block = :auto, ngpus = 8)`).
 * Needs `opt->row_block` or `opt->detect_blocks`; K1 or K2; `opt->refine_steps` is honoured (K1).  devices: ngpus HIP ordinals, or
 * NULL for 0 .. ngpus-1 (an ordinal may repeat: several shards on one device, for testing).  One host analyse serves all shards; the
 * two reductions of a Newton step (root panel, root right-hand side) are done inside the library, stream-ordered -- peer-to-peer
 * copies + an ordered sum on devices[0], or ncclAllReduce (librccl.so through dlopen) with TLPK_MULTI_REDUCE=rccl --; results are
 * gathered on devices[0].  The handle accepts tlpk_update / tlpk_solve / tlpk_sync / tlpk_info / tlpk_get_perm / tlpk_destroy and the
 * device-resident loops (tlpk_ipm_*, tlpk_mpc_*); the device-pointer and split-phase calls belong to single and sharded handles. */
int tlpk_create_multi(tlpk_handle **out, int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval,
                      const double *nzval, int index_base, const tlpk_options *opt, int ngpus, const int32_t *devices);

/* Block-angular structure of an m x n CSC matrix (int64 indices, index_base in {0,1}): row_block[i] = block id >= 0 of row i,
 * or -1 for a linking row -- the vector tlpk_options.row_block takes.  Rows are adjacent when they share a column; the densest
 * rows are removed (at most max_link_rows, 0 = max(64, m / 20)) until no connected component of the rest holds more than half of
 * the remaining rows -- or, for an LP with one dominant block, at most 80 % of them next to a second component of block size
 * (TLPK_DETECT_MAX_FRACTION) --; a small such set of linking rows is found by a geometric probe + bisection (the acceptance test is not
 * monotone in the number of removed rows, so "small", not "smallest"); small components (isolated rows) are packed into the blocks.  *n_blocks = number of diagonal blocks, 1 = no block structure (then every row_block[i] = 0 and the caller should
 * pass row_block = NULL).  Host only, deterministic, O(nnz log max_link_rows).  n_blocks / n_link may be NULL. */
int tlpk_detect_blocks(int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval, int index_base,
                       int64_t max_link_rows, int64_t *row_block /*m*/, int64_t *n_blocks, int64_t *n_link);

/* Introspection */
int tlpk_info(const tlpk_handle *h, tlpk_stats *out);
int tlpk_kernel_timing(const tlpk_handle *h, tlpk_kernel_times *out);
int tlpk_set_profile(tlpk_handle *h, int on);   /* toggle per-launch HIP-event timing at run time; while on, the
                                                   stream groups are serialised on the main stream so that the
                                                   per-kernel durations are not inflated by overlap */
int tlpk_get_perm(const tlpk_handle *h, int64_t *perm /*m, 0-based, perm[new] = old*/);   /* dense_cols: the constraint nodes in their order
                                                   (the whole order-(m + k) permutation: tlpk_symbolic_get(h, "perm"), node m + t = dense column t) */
/* Symbolic structures, for tests and tools.  `what` selects an array; returns its length and,
 * if buf != NULL, copies min(len, cap) int64 entries.  One key is a counter, not a structure: "krylov_unsolved" (matrix-free handles; see tlpk_stats); "krylov_pair" holds the
 * counters of tlpk_solve2_device on such a handle (see "pair" at tlpk_options.krylov), and tlpk_symbolic_get_f64 serves "krylov_pair_resid" beside "pair_w".
 * Read-only diagnostics of the launch schedule (tests/test_schedule_identity.py):
 *   "launch_meta"  (stream group, side, pad) of every entry of "factor_launches", then of "fwd_launches", then of "bwd_launches"
 *   "zero_tasks"   (front, first column) of every 64-column panel slice the zero-fill clears
 *   "zero_small"   the fronts whose whole panel one wave clears
 *   "singles"      panel offsets, inverted-diagonal offsets and columns of the isolated 1 x 1 fronts, concatenated; then n_zero_lower and spart_len
 * Launch geometry of a dense-matrix handle (tlpk_create_dense; tests/test_dense_shapes.py), six entries, all zero on any other handle:
 *   "dense_geometry"  [0] syrk_split   K (= n) parts per 128 x 128 tile of A D A' (1: the tiles go straight into the panel, no reduction)
 *                     [1] syrk_kc      columns per part, a multiple of 16: part p = columns [p kc, min(n, (p + 1) kc))
 *                     [2] gemv_chunks  column chunks of xi_p + A (D .* xi_d), whose partial sums are added in chunk order (>= 1)
 *                     [3] gemv_cw      columns per chunk: chunk c = columns [c cw, min(n, (c + 1) cw))
 *                     [4] dense_lda    leading dimension of the device copy of A (m rounded up to 16; the padding rows are zero)
 *                     [5] panel_lda    leading dimension of the one front's packed panel (= "front_lda"[0])
 *                     -- the values the kernels receive: a device handle is created from these numbers, not from a second computation */
int64_t tlpk_symbolic_get(const tlpk_handle *h, const char *what, int64_t *buf, int64_t cap);
int64_t tlpk_symbolic_get_f64(const tlpk_handle *h, const char *what, double *buf, int64_t cap);
/* Copy the numeric factor panels (device -> host), nnzL_stored doubles.  Layout: front s (symbolic arrays front_f, front_ns, front_loff,
 * front_lda) stores its f x ns panel column-major by 64-column slices -- slice b = columns [64 b, 64 b + 64) from row 64 b down, leading
 * dimension lda - 64 b; entry (row, col) at loff + col * lda - 64 b (col - 32 b - 31) + row, b = col / 64 (fronts of <= 64 pivot
 * columns: plain column-major with leading dimension lda). */
int tlpk_get_factor(tlpk_handle *h, double *lval, int64_t cap);

/* ---------------------------------------------------------------------------------------------
 * Block skip: leave diagonal blocks out of the following updates and solves (DESIGN.md section 4b'-s).  A handle whose matrix is block
 * diagonal (tlpk_options.row_block, no linking rows) factorises and solves its blocks independently: no front of one block shares data
 * with a front of another.  skip[k] != 0: block k (the ids of tlpk_options.row_block) is skipped; skip == NULL: no mask.  The mask
 * stays in force until it is replaced.  It is a runtime predicate: the launch schedules, grids and task lists are what they are without
 * it, the workgroups of a skipped block return at once, and nothing a skipped block owns is read or written.
 *   Update.  The skipped blocks' panels, inverted diagonal blocks and update buffers keep every bit (they are not zeroed either); the
 *   other blocks' factor equals an unmasked update's bit for bit.  A non-positive pivot in a skipped block cannot fail the update:
 *   tlpk_stats.fail_col can only name a column of a block that ran.
 *   Solve.  The other blocks' segments of dx / dy equal an unmasked solve's bit for bit (tlpk_solve_device and both right-hand sides of
 *   tlpk_solve2_device; the host-pointer calls run the same kernels).  The segments of the skipped blocks are unspecified, but finite for
 *   finite input and never uninitialised memory.  A block that is solved must have been factorised by the last update that touched it:
 *   that is the caller's contract -- violating it gives unspecified values, never a wait.  After tlpk_block_skip(h, NULL, n_blocks) the
 *   handle behaves as if no mask had ever been set.
 *   Graph replay.  tlpk_set_values*, replayed schedules and tlpk_update_device_async keep working: the mask's content is read when the
 *   kernels run, so a captured schedule stays valid when the mask changes.
 * Checks, in this order (TLPK_BADARG with a sentence in tlpk_last_error unless a code is named): h NULL; not a single-device direct handle
 * (multi-device, sharded, dense-matrix, Krylov and dense_cols handles); refine_steps > 0 (the refinement's norms run over all rows); a
 * batch-loaded handle (the batch owns the mask: tlpk_ipm_batch_skip); no row_block, or linking rows; nblocks != tlpk_stats.n_blocks; a
 * front that is not contained in one block (its pivot columns, its row indices, its parent); then TLPK_NO_DEVICE on an analyse-only
 * handle.  A failed call leaves the previous mask in force.
 * tlpk_symbolic_get keys: "front_unit" the block of every front, then of every isolated 1 x 1 front in the order of "singles" (-1 before
 * the table exists: it is built by the first call that reaches that check); "front_skip" the bytes in force, per front and then per
 * single (empty = no mask); "skip_bytes" one entry, the device memory of the tables (part of tlpk_stats.device_bytes once allocated).
 * --------------------------------------------------------------------------------------------- */
int tlpk_block_skip(tlpk_handle *h, const uint8_t *skip /*nblocks*/, int64_t nblocks);

/* ---------------------------------------------------------------------------------------------
 * Device-resident HSD iterate: an OPTIONAL extension for callers that keep the
 * interior-point vectors in HBM.  The drop-in interface above moves 16 (m + n) bytes over PCIe per
 * solve and leaves every right-hand side to the host; here one call runs one routine of
 * /root/reference/src/IPM/HSD/{HSD.jl, step.jl} on device vectors owned by the handle and returns only
 * scalars.  The host keeps tau, kappa, the regularisation scalars and the control flow
 * (tulip.jl_amd/hsd_device.py mirrors HSD.jl:203-350).
 * Handles: one rank, or a tlpk_create_multi handle (K1 or K2 either way).  On several devices every shard holds the sub-LP of its
 * diagonal blocks in vectors of the job's length (its columns with costs and bounds, its block rows of b, the linking rows with b
 * on the lead shard and A restricted to its columns): the same kernels then produce each shard's share of every sum / maximum /
 * minimum, the host combines them in shard order, the KKT solves run split-phase with every shard's partial xi_p on the linking
 * rows (the library's reduction of the root right-hand side completes them), and |rp|inf, |A x|inf on the linking rows come from
 * the shards' partial rows summed on the host.  The iterates equal the single-device ones up to the re-association of those
 * sums.  Sharded handles (nranks > 1) are refused: their reductions belong to the caller.
 * --------------------------------------------------------------------------------------------- */
/* b (m), c (n), l, u (n; +-Inf allowed) of the standard form (ipmdata.jl:64-173); sets the HSD starting point
 * (HSD.jl:238-247).  tlpk_ipm_reset restores the starting point. */
int tlpk_ipm_load(tlpk_handle *h, const double *b, const double *c, const double *l, const double *u);
int tlpk_ipm_reset(tlpk_handle *h);
/* New LP data on a handle that has been tlpk_ipm_load'ed (typically after tlpk_set_values*): refreshes the copies of A the loops keep, takes the vectors
 * that are not NULL (NULL = keep), recomputes the finite-bound flags -- bounds may change between finite and infinite -- and restores the HSD starting
 * point.  The device vectors are reused: tlpk_stats.device_bytes does not grow.  All four NULL: same data, new A, start over.  A handle that was never
 * loaded: TLPK_BADARG (call tlpk_ipm_load first). */
int tlpk_ipm_reload(tlpk_handle *h, const double *b, const double *c, const double *l, const double *u);
/* HSD.jl:77-128, 136-196.  out[13] = { |rp|inf, |rl|inf, |ru|inf, |rd|inf, c'x, b'y, lz'zl, uz'zu, xl'zl + xu'zu,
 *                                      |Ax|inf, |(x-xl) lflag|inf, |(x+xu) uflag|inf, |A'y + zl lflag - zu uflag|inf } */
int tlpk_ipm_residuals(tlpk_handle *h, double tau, double *out);
/* step.jl:24-51: theta_inv from the iterate, uniform regP / regD, KKT.update!; TLPK_NOT_POSDEF -> retry with larger values */
int tlpk_ipm_factor(tlpk_handle *h, double regP, double regD);
/* step.jl:56-76: h-system; out[0] = lz'(lz th_l) + uz'(uz th_u) - (c + th_l lz + th_u uz)'hx + b'hy */
int tlpk_ipm_hsolve(tlpk_handle *h, double *out);
/* step.jl:325-364: centrality targets from the accepted direction; out[2] = { sum(vl), sum(vu) } */
int tlpk_ipm_targets(tlpk_handle *h, double a_, double mu_l, double mu_u, double *out);
/* step.jl:198-266 + 294-306: one Newton system.  mode 0 predictor | 1 corrector | 2 centrality corrector;
 * sc[8] = { tau, kappa, h0, xi_g, xi_tk, eta, gamma*mu, delta }; out[3] = { dtau, dkappa, max step to the boundary } */
int tlpk_ipm_newton(tlpk_handle *h, int mode, const double *sc, double *out);
/* step.jl:56-94: tlpk_ipm_hsolve + tlpk_ipm_newton(mode 0) with the two independent solves sharing one pass over the factor
 * (tlpk_solve2_device).  sc[8] as above except sc[2] = regG (h0 is formed inside); out[4] = { dtau, dkappa, max step, h0 } */
int tlpk_ipm_hsolve_newton(tlpk_handle *h, const double *sc, double *out);
/* step.jl:24-94: tlpk_ipm_factor without the wait for its status + tlpk_ipm_hsolve_newton: the paired solve's block-level forward sweeps
 * overlap the factorisation of the root front (tlpk_update_device_async); returns TLPK_NOT_POSDEF where tlpk_ipm_factor would have */
int tlpk_ipm_factor_hsolve_newton(tlpk_handle *h, double regP, double regD, const double *sc, double *out);
/* Refinement inside the loops, switched at run time (single-device handles with a factor and ONE LP loaded; anything else TLPK_BADARG with a sentence, an
 * analysis-only handle TLPK_NO_DEVICE): from now on every KKT solve inside tlpk_ipm_hsolve, _newton, _hsolve_newton, _factor_hsolve_newton, tlpk_mpc_start and
 * tlpk_mpc_newton is followed by `steps` steps of tlpk_polish_device on the same vectors -- the pair of _hsolve_newton by tlpk_polish2_device, so that the
 * refined pair still makes paired passes over L.  steps = 0 restores the plain calls bit for bit.  K1 and K2. */
int tlpk_ipm_set_polish(tlpk_handle *h, int steps);
int tlpk_ipm_accept(tlpk_handle *h);                         /* step.jl:112-118: candidate -> accepted direction */
int tlpk_ipm_advance(tlpk_handle *h, double alpha, double *out);   /* step.jl:139-148; out[0] = xl'zl + xu'zu */
/* Read one device vector (nothing is written on the device; there is no setter).  `len` must be the vector's length.
 *   what  0-5    the iterate x, xl, xu, zl, zu (n), y (m)
 *         6-11   the accepted direction, same order;  12-17  the candidate direction of the last mode-2 call, same order
 *         18-21  the residuals rp (m), rl, ru, rd (n)
 *         22-26  thl, thu, hx (n), hy (m), hxid (n): the two halves of theta_inv, the solution and the dual right-hand side of the h-system
 *         27-32  xil, xiu, xzl, xzu, xid (n), xip (m): the right-hand sides of the last Newton system (xzl / xzu: the targets after tlpk_ipm_targets)
 *         33-35  theta_inv (n), regP (n), regD (m) as the last factor call wrote them on the handle
 * Codes 0-5 serve every handle with a loaded LP; 6-35 single-device handles only (batch-loaded ones included: the stacked vectors) --
 * on a multi-device handle they return TLPK_BADARG with a sentence in tlpk_last_error.  Any other code: TLPK_BADARG.
 * The codes above 5 exist for tests (tests/test_ipm_kernels.py reads every kernel's output through them). */
int tlpk_ipm_get(tlpk_handle *h, int what, double *host, int64_t len);

/* ---------------------------------------------------------------------------------------------
 * Batched device-resident HSD: MANY SMALL LPs in one set of launches.  B LPs stacked into one block-diagonal A are an ordinary handle
 * (row_block = LP index and no linking rows: the analysis is a forest, the level-batched kernels serve every block in the launches one
 * block needs).  tlpk_ipm_load_batch takes the place of tlpk_ipm_load on such a handle and the tlpk_ipm_batch_* calls run the routines
 * above with PER-LP scalars: LP k owns the contiguous rows [row_off[k], row_off[k+1]) and columns [col_off[k], col_off[k+1]) of the
 * stacked vectors, every array argument below has one entry (or one group of entries) per LP, and an LP with active[k] = 0 is not
 * touched: nothing writes its iterate, direction, h-system or right-hand sides (the KKT solves of these calls write scratch vectors and only
 * the active LPs take their segments), its outputs are 0.  The reductions of an LP do not depend on
 * what else is in the batch; with nlp = 1 every call returns what its unbatched counterpart returns, bit for bit.
 *   tlpk_ipm_load_batch checks, in this order (TLPK_BADARG with a sentence in tlpk_last_error): pointers not NULL and nlp >= 1; offsets
 *   start at 0, do not decrease, leave no LP without rows or columns and end at m and n; every stored entry of A lies in its LP's diagonal
 *   block; the handle is a single-device direct one (K1 or K2; row_block and refine_steps are fine; multi-device, sharded, dense-matrix,
 *   Krylov and dense_cols handles are refused); nothing is loaded yet (either load after the other: TLPK_BADARG).  Then TLPK_NO_DEVICE on
 *   an analyse-only handle.
 *   tlpk_ipm_reset, tlpk_ipm_reload and tlpk_ipm_get serve a batch-loaded handle unchanged (stacked vectors); every other tlpk_ipm_* /
 *   unbatched tlpk_mpc_* call on it returns TLPK_BADARG, as does every tlpk_ipm_batch_* / tlpk_mpc_batch_* call on a handle loaded with
 *   tlpk_ipm_load (or not loaded).
 *   tlpk_ipm_batch_factor: regP[k] / regD[k] are uniform within LP k.  An LP with active[k] = 0 is PARKED: theta_inv = 1, Rp = Rd = 1 on
 *   its block (the matrix the handle is analysed with), so a finished or failed LP cannot fail the update of the others.  Whether the
 *   parked block is then factorised and swept like every other block (the default) or left out of the update and the solves is
 *   tlpk_ipm_batch_skip's choice, below; the vectors read with codes 33 - 35 of tlpk_ipm_get hold the parking values either way.  On
 *   TLPK_NOT_POSDEF *fail_lp is the LP that owns tlpk_stats.fail_col (through the permutation; K2: node j < n is a column, n + i a row),
 *   or -1 if that cannot be told; one failure is reported per update.  Otherwise *fail_lp = -1.
 * --------------------------------------------------------------------------------------------- */
int tlpk_ipm_load_batch(tlpk_handle *h, int64_t nlp, const int64_t *row_off /*nlp+1*/, const int64_t *col_off /*nlp+1*/,
                        const double *b, const double *c, const double *l, const double *u);   /* stacked, lengths m, n, n, n */
int tlpk_ipm_batch_residuals(tlpk_handle *h, const double *tau /*nlp*/, double *out /*13 nlp, the layout of tlpk_ipm_residuals per LP*/);
int tlpk_ipm_batch_factor(tlpk_handle *h, const uint8_t *active, const double *regP /*nlp*/, const double *regD /*nlp*/, int64_t *fail_lp);
/* sc[8 k ..], out[4 k ..]: as tlpk_ipm_hsolve_newton for LP k */
int tlpk_ipm_batch_hsolve_newton(tlpk_handle *h, const uint8_t *active, const double *sc /*8 nlp*/, double *out /*4 nlp*/);
/* one mode for the call; sc[8 k ..], out[3 k ..]: as tlpk_ipm_newton for LP k */
int tlpk_ipm_batch_newton(tlpk_handle *h, int mode, const uint8_t *active, const double *sc /*8 nlp*/, double *out /*3 nlp*/);
int tlpk_ipm_batch_targets(tlpk_handle *h, const uint8_t *active, const double *par /*3 nlp: a_, mu_l, mu_u*/, double *out /*2 nlp*/);
/* the candidates of the LPs with active[k] != 0 become their accepted directions (a copy: the LPs accept independently) */
int tlpk_ipm_batch_accept(tlpk_handle *h, const uint8_t *active);
int tlpk_ipm_batch_advance(tlpk_handle *h, const uint8_t *active, const double *alpha /*nlp*/, double *out /*nlp*/);
/* Batch-loaded handles: on != 0 -> every tlpk_ipm_batch_* / tlpk_mpc_batch_* call that takes `active` skips the blocks of the LPs with
 * active[k] == 0 in its update / its solves (tlpk_block_skip's mechanism with the LPs as blocks; the flags travel with the call's scalars,
 * there is no extra copy).  Default 0 = every block is factorised and swept.  With it on, tlpk_ipm_batch_factor still writes the parking
 * values and leaves the parked LPs' panels as they are; tlpk_ipm_batch_hsolve_newton, tlpk_ipm_batch_newton and tlpk_mpc_batch_newton
 * skip the parked LPs in their solves (an LP that is solved must be active in the last tlpk_ipm_batch_factor that followed its last change:
 * the loops of hsd_batch.py / mpc_batch.py factorise every LP they solve).  tlpk_mpc_batch_start and tlpk_ipm_batch_refill run unmasked,
 * and outside these calls no mask is in force.  The active LPs' results do not depend on the setting, bit for bit.
 * TLPK_BADARG on a handle that is not batch-loaded, on one with refine_steps > 0, or when an LP's fronts are not its own. */
int tlpk_ipm_batch_skip(tlpk_handle *h, int on);
/* One update of the stack with a ROLE per LP and a VERDICT per LP: every LP whose block meets a non-positive pivot is reported by the
 * one call, and an LP that already holds a good factor can keep it while the others are factorised again.  role[k]:
 *   0  parked    the parking values, as active[k] = 0 of tlpk_ipm_batch_factor; whether the parked block is factorised stays
 *                tlpk_ipm_batch_skip's choice
 *   1  active    theta_inv from the iterate, regP[k] / regD[k], factorised: tlpk_ipm_batch_factor's active LP
 *   2  hold      nothing of the LP is written, assembled, zeroed or factorised: its segments of the vectors behind codes 33 - 35 of
 *                tlpk_ipm_get, its panels and its inverted diagonal blocks keep every bit, regP[k] / regD[k] are not read, and the factor
 *                of an earlier call stays the one the next solves use (tlpk_block_skip's mechanism, whatever tlpk_ipm_batch_skip says)
 *   3  entering  what tlpk_mpc_batch_factor_enter does for enter[k]
 * fail_col[k] = the permuted column of LP k's first non-positive pivot in this update, or -1; *nfail = the number of LPs with one.  A held
 * or parked-and-skipped LP never has one.  TLPK_OK: no LP failed, the handle is factored.  TLPK_NOT_POSDEF: at least one did, the handle
 * is not factored (as after tlpk_ipm_batch_factor), tlpk_stats.fail_col is the smallest of them; the blocks of the other LPs hold valid
 * factors -- a failing pivot is replaced by 1 inside its own block -- which a following call can hold.  After the call no mask is in force.
 * An update without a failure costs no extra copy and no extra wait.
 * TLPK_BADARG, in this order: h NULL; a handle that is not batch-loaded; a NULL pointer; a role above 3; a stale handle after
 * tlpk_set_values*; ("... hold refused: ...") a hold on a handle with refine_steps > 0 or on one where an LP's fronts are not its own (tlpk_ipm_batch_skip's
 * conditions, but for one case: a front that LPs share and that stands alone -- no rows below its pivot block, no children; K2 gathers the
 * columns of A without entries in such a root front -- is accepted and factorised by every call, holds or not).  Then TLPK_NO_DEVICE. */
int tlpk_ipm_batch_factor_each(tlpk_handle *h, const uint8_t *role /*nlp*/, const double *regP /*nlp*/, const double *regD /*nlp*/,
                               int64_t *fail_col /*nlp*/, int64_t *nfail);

/* ---------------------------------------------------------------------------------------------
 * Refilling slots: a batch that keeps going.  A batch-loaded handle has nlp SLOTS; when the LP of a slot is decided, the next LP of the
 * caller's queue with the same pattern takes the slot while every other slot continues, so N LPs stream through one analysed handle
 * (tulip.jl_amd/hsd_batch.py: BatchedDeviceHSD.optimize_stream).
 *   tlpk_ipm_batch_refill replaces the LPs of the slots with slots[k] != 0: tlpk_set_values + tlpk_ipm_reload restricted to those LPs.
 *   nzval (nnzA, the STACKED matrix in the caller's CSC order) or NULL = keep A; b (m), c, l, u (n) stacked, each may be NULL = keep.  Only
 *   the selected LPs' segments of the arrays are read, and only those reach the device.  For the selected LPs it rewrites the values of
 *   their columns of A and everything derived from them (the products of the assembly lists, the value arrays of every copy of A the handle
 *   keeps; K2: the incidence copy and the copies the loops keep), their segments of b, c, l, u, their finite-bound flags (bounds may change
 *   between finite and infinite) and their iterate, which becomes the HSD starting point of tlpk_ipm_reset.  Their parts of the handle then
 *   equal, bit for bit, those of a handle created and batch-loaded on the stacked data with these LPs in place.  An LP that is not
 *   selected keeps every bit: its segment of every vector tlpk_ipm_get reads, its columns' values, its derived arrays.  With new values
 *   the handle is analysed but not factored afterwards, as after tlpk_set_values: the next tlpk_ipm_batch_factor factorises.
 *   Checks, in this order (TLPK_BADARG): h NULL; not batch-loaded (the "load first" sentence of the tlpk_ipm_batch_* calls); slots NULL;
 *   nzval given with len != nnzA; the handle is stale after a whole-handle tlpk_set_values* without tlpk_ipm_reload.  A failed check leaves
 *   the handle as it was; no slot selected: TLPK_OK and nothing happens.  K1 and K2; refine_steps and row_block are fine, as at load.
 *   The Mehrotra batch refills with the same call; the starting point of the new LPs (a factorisation and two solves per LP) then rides in the
 *   update and the solves of the running LPs: "Entering LPs" below.
 *   tlpk_ipm_get_lp is tlpk_ipm_get for ONE LP of a batch-loaded handle: LP k's segment of vector `what` (the codes of tlpk_ipm_get), len =
 *   that segment's length.  Refusals as tlpk_ipm_get, plus TLPK_BADARG on a handle that is not batch-loaded, k out of range, a wrong len.
 *   tlpk_ipm_get_lps reads the records of the LPs that leave in one go: the segments of the nwhat codes what[] (any order, row and column
 *   vectors mixed) for the nk LPs lp[] (any order, each at most once), LP-major with the codes in the given order, len = the sum of the
 *   segments' lengths.  One kernel gathers the segments into a device staging buffer (allocated by the first call, grown by a larger one; the
 *   segment table travels with the launch), one copy brings them to `host`: the bytes are those of the tlpk_ipm_get_lp calls it replaces.
 *   Refusals as tlpk_ipm_get_lp (NULL pointers and a code outside 0 .. 35 included), plus TLPK_BADARG with a sentence on an LP out of range, an
 *   LP listed twice, a wrong len.  nk = 0 or nwhat = 0 with len = 0: TLPK_OK, nothing is written.
 * --------------------------------------------------------------------------------------------- */
int tlpk_ipm_batch_refill(tlpk_handle *h, const uint8_t *slots /*nlp*/, const double *nzval, int64_t len,
                          const double *b, const double *c, const double *l, const double *u);
int tlpk_ipm_get_lp(tlpk_handle *h, int what, int64_t k, double *host, int64_t len);
int tlpk_ipm_get_lps(tlpk_handle *h, const int32_t *what, int64_t nwhat, const int64_t *lp, int64_t nk, double *host, int64_t len);

/* ---- Mehrotra predictor-corrector with the iterate in HBM (/root/reference/src/IPM/MPC/MPC.jl:218-410,
 * MPC/step.jl:10-358).  Same vectors as above: tlpk_ipm_load once, tlpk_ipm_residuals with tau = 1 (MPC.jl:101-141),
 * tlpk_ipm_factor (step.jl:24-51), tlpk_ipm_accept and tlpk_ipm_get are shared. */
int tlpk_mpc_start(tlpk_handle *h, double *out);               /* MPC.jl:353-410 starting point; out[0] = xl'zl + xu'zu */
/* mode 0 predictor | 1 corrector (gmu = sigma mu) | 2 centrality corrector; out[0], out[1] = largest primal / dual step
 * to the boundary of the written direction (inf if unbounded)   MPC/step.jl:164-217 */
int tlpk_mpc_newton(tlpk_handle *h, int mode, double gmu, double *out);
/* out[0] = complementarity at the point moved by (ap, ad) along the accepted direction, out[1] = at the point   step.jl:246-258 */
int tlpk_mpc_gap(tlpk_handle *h, double ap, double ad, double *out);
int tlpk_mpc_targets(tlpk_handle *h, double ap_, double ad_, double tmin, double tmax);      /* step.jl:329-358 */
int tlpk_mpc_advance(tlpk_handle *h, double ap, double ad, double *out);                     /* step.jl:112-123; out[0] = xl'zl + xu'zu */

/* ---------------------------------------------------------------------------------------------
 * Batched device-resident MPC: the tlpk_mpc_* calls above on a handle loaded with tlpk_ipm_load_batch, with PER-LP scalars and the
 * `active` masks of the tlpk_ipm_batch_* calls (an LP with active[k] = 0 is not touched and its outputs are 0; with nlp = 1 every call
 * returns what its unbatched counterpart returns, bit for bit).  Shared with the HSD batch as they are: tlpk_ipm_batch_residuals with
 * tau[k] = 1, tlpk_ipm_batch_factor (parking included), tlpk_ipm_batch_accept, tlpk_ipm_get, tlpk_ipm_reset / tlpk_ipm_reload.
 * Refusals as the tlpk_ipm_batch_* calls: TLPK_BADARG with a sentence in tlpk_last_error on a handle that is not loaded or loaded with
 * tlpk_ipm_load, on NULL pointers, on a mode outside 0 .. 2 and after tlpk_set_values without tlpk_ipm_reload; TLPK_NO_DEVICE on an
 * analyse-only handle.
 *   tlpk_mpc_batch_start: every LP is active; a failed update returns its code, as tlpk_mpc_start does.
 * --------------------------------------------------------------------------------------------- */
int tlpk_mpc_batch_start(tlpk_handle *h, double *out /*nlp: xl'zl + xu'zu*/);
/* one mode for the call; out[2 k ..] = largest primal / dual step to the boundary of LP k's written direction (inf if unbounded) */
int tlpk_mpc_batch_newton(tlpk_handle *h, int mode, const uint8_t *active, const double *gmu /*nlp*/, double *out /*2 nlp*/);
int tlpk_mpc_batch_gap(tlpk_handle *h, const uint8_t *active, const double *ap /*nlp*/, const double *ad /*nlp*/, double *out /*2 nlp*/);
int tlpk_mpc_batch_targets(tlpk_handle *h, const uint8_t *active, const double *par /*4 nlp: ap_, ad_, tmin, tmax*/);
int tlpk_mpc_batch_advance(tlpk_handle *h, const uint8_t *active, const double *ap /*nlp*/, const double *ad /*nlp*/, double *out /*nlp*/);

/* ---------------------------------------------------------------------------------------------
 * Entering LPs: the Mehrotra batch as a stream (tulip.jl_amd/mpc_batch.py: BatchedDeviceMPC.refill / optimize_stream; DESIGN.md 4b''-s).
 * The starting point of tlpk_mpc_batch_start costs one factorisation and two solves.  For an LP that tlpk_ipm_batch_refill has just put into
 * a slot none of them needs launches of its own: a stacked update factorises every block with that block's own values and a stacked solve
 * takes a right-hand side per block, so the LP ENTERS through the update, the predictor solve and the corrector solve of the LPs that are
 * running.  The three calls carry an `enter` mask beside `active`; both are arguments of every call, nothing is remembered on the handle.
 *   tlpk_mpc_batch_factor_enter  = tlpk_ipm_batch_factor for the active and the parked LPs (neither flag: parked).  An entering LP gets what
 *     tlpk_mpc_batch_start writes before its update: theta_inv = 0, Rp = 1, xid = hx = 0 on its columns, Rd = 1e-6, xip = hy = 0 on its rows.
 *     With tlpk_ipm_batch_skip on, the update leaves out the LPs that are neither active nor entering.  *fail_lp may name an entering LP.
 *   tlpk_mpc_batch_newton_enter  = tlpk_mpc_batch_newton(mode 0 | 1) for the active LPs.  For an entering LP the segment of the right-hand
 *     side of the call's one stacked solve is (xip, xid) = (0, c) with mode 0, its solution goes to (the accepted direction's x, y); with mode 1
 *     it is (b, 0) and goes to (x, the accepted direction's y) -- the two solves of tlpk_mpc_batch_start, in its order.  The half of the
 *     right-hand side that was used is 0 again afterwards.  out of an entering LP is 0.  The solve leaves out the LPs that are neither active
 *     nor entering (tlpk_ipm_batch_skip).  mode 2: TLPK_BADARG (the centrality correctors keep using tlpk_mpc_batch_newton, which does not
 *     touch an entering LP).
 *   tlpk_mpc_batch_enter_finish  runs the rest of the starting point (shifts to positive coordinates, balanced products) on the entering LPs
 *     alone; out[k] = xl'zl + xu'zu of LP k's starting point, 0 for every other LP.  From the next call on the LP is an active one.
 * Contracts, bit for bit: with enter all zero each call is its counterpart (outputs and every vector tlpk_ipm_get reads); with every LP
 * entering and none active, factor_enter, newton_enter(0), newton_enter(1), enter_finish is tlpk_mpc_batch_start (out and the codes 0 - 32);
 * an entering LP's results do not depend on what the other LPs of the call are or do, nor theirs on it; an LP that is neither active nor
 * entering keeps every bit of the codes 0 - 32.
 * Refusals, in this order: TLPK_BADARG with a sentence on a handle that is not loaded or loaded with tlpk_ipm_load, on NULL pointers, after
 * tlpk_set_values without tlpk_ipm_reload; TLPK_BADARG with a sentence when an LP is both active and entering (and on mode 2); then
 * TLPK_NO_DEVICE.
 * --------------------------------------------------------------------------------------------- */
int tlpk_mpc_batch_factor_enter(tlpk_handle *h, const uint8_t *active, const uint8_t *enter, const double *regP /*nlp*/, const double *regD /*nlp*/,
                                int64_t *fail_lp);
int tlpk_mpc_batch_newton_enter(tlpk_handle *h, int mode /*0 | 1*/, const uint8_t *active, const uint8_t *enter, const double *gmu /*nlp*/,
                                double *out /*2 nlp*/);
int tlpk_mpc_batch_enter_finish(tlpk_handle *h, const uint8_t *enter, double *out /*nlp: xl'zl + xu'zu*/);

const char *tlpk_strerror(int code);
const char *tlpk_last_error(const tlpk_handle *h);
/* message of the last FAILED tlpk_create / tlpk_create_multi of the calling thread ("" after a successful one): a failed create returns no handle */
const char *tlpk_last_create_error(void);
const char *tlpk_backend_name(void);         /* "HIP (gfx950)" */
const char *tlpk_system_name(void);          /* "Normal equations (K1)" */
const char *tlpk_linear_system(const tlpk_handle *h);   /* KKT.linear_system of this handle: "... (K1)" | "Augmented system (K2)" */
int tlpk_device_count(void);
/* host threads (pool workers + the caller) that stage the vectors of the host-pointer calls tlpk_update / tlpk_solve through pinned memory;
 * TLPK_COPY_THREADS = number of workers (default 4, 0 = the caller copies alone), read when the pool is first used */
int tlpk_host_copy_threads(void);

#ifdef __cplusplus
}
#endif
#endif /* TLPK_H */
