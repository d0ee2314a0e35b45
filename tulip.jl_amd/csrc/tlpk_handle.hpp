// tlpk_handle.hpp -- the solver object behind `tlpk_handle*` and the small helpers shared by the
// translation units of the C ABI (tlpk_api.cpp: KKT interface; tlpk_ipm.cpp: device-resident IPM vectors).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <array>
#include <vector>

#include "../../include/tlpk.h"
#include "tlpk_device.hpp"

using namespace tlpk;

struct IpmState;        // tlpk_ipm.cpp
constexpr int MAX_DEVICES = 16;

struct tlpk_handle {
    Symbolic S;
    Options opt;
    std::vector<i64> row_block_copy, user_perm_copy;
    int device = -1;
    bool has_device = false;
    bool profile = false;
    int fault_at = -1, n_updates = 0; bool fault_done = false;      // TLPK_CHAIN_FAULT (testing): see enq_update_local
    int chain_retries = 0;        // tlpk_update: replays after a dependency-driven launch gave up waiting
    bool shared_device = false;   // set by tlpk_create_multi when another shard of the job names the same device (Options::shared_device)
    bool serial = false;          // TLPK_SERIAL=1: every launch on the main stream (what profile mode does), for external profilers
    hipStream_t stream = nullptr;                 // main stream (= group 0)
    hipStream_t gstream[MAX_GROUPS] = {};         // gstream[0] == stream; others: concurrent subtree groups
    hipEvent_t ev_fork = nullptr, ev_join[MAX_GROUPS] = {};
    hipStream_t zstream = nullptr;        // lowest priority: the upper fronts' zero-fill + assembly must not take slots from the leaf levels' launches
    hipEvent_t ev_zfork = nullptr, ev_upper = nullptr;   // zero-fill + assembly of the upper fronts beside the leaf levels (schedule.cpp, step 13d)
    bool upper_split = false;             // this update runs them on the last group's side stream (set per call: not in the single-stream modes / graphs)
    hipStream_t sstream[MAX_GROUPS] = {};         // side stream of each group: diagonal-block chains overlap the bulk update
    hipEvent_t ev_side[MAX_GROUPS] = {};
    bool forked = false;
    hipStream_t rstream = nullptr;                // the root (linking) front of tlpk_update_device_async runs here, beside the next solve's block sweeps
    hipEvent_t ev_blocks = nullptr, ev_root = nullptr;
    bool root_pending = false;                    // an asynchronous update has not been waited for / checked yet
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<hipEvent_t> ev_pool;
    std::vector<int> ev_class;            // class of each recorded pair in the current call
    std::vector<std::array<long long, 3>> ev_launch;   // (kind, first, count) of the launch behind each pair (-1: not a schedule launch): TLPK_PROF_DUMP
    size_t ev_used = 0;
    DevArrays d;
    std::vector<EaGatherLaunch> eg_launches;      // the LK_EXTEND_ADD launches with a gathered front (d.eg_launch points here)
    std::vector<void *> allocs;
    i64 device_bytes = 0;
    double *d_theta = nullptr, *d_regP = nullptr, *d_regD = nullptr, *d_D = nullptr;
    double *d_xip = nullptr, *d_xid = nullptr, *d_dx = nullptr, *d_dy = nullptr;
    int refine_steps = 0;                         // tlpk_options.refine_steps
    double *d_r1 = nullptr, *d_r2 = nullptr, *d_cx = nullptr, *d_cy = nullptr;   // refinement: residuals and correction
    unsigned long long *d_ref = nullptr;          // guarded refinement: norms and verdict words (kernels.hip: k_refine_decide)
    i64 refine_rejected = 0;                      // refinement steps of the last solve that did not shrink the residual and were discarded
    double *d_bx = nullptr, *d_by = nullptr;      // multi-device refinement: the iterate before a step (restored if the step is rejected)
    // refinement on demand (tlpk_polish_device / tlpk_polish2_device; tlpk_api.cpp: polish_*), everything allocated by the first call: residuals and
    // corrections of two systems, the state words of both (tlpk_device.hpp: PolishWord) and their pinned copy, K2: the device copies of A
    struct Polish {
        double *r1[2] = {nullptr, nullptr}, *r2[2] = {nullptr, nullptr}, *cx[2] = {nullptr, nullptr}, *cy[2] = {nullptr, nullptr};
        unsigned long long *d_ref = nullptr, *h_ref = nullptr;
        bool ready = false, pair_ready = false;   // the first set / the second set (allocated by the first pair) is there
        PolishMat A{};                            // K1: the handle's own copies; K2: own copies, or the loops' (tlpk_ipm_load)
        bool own_A = false, A_ready = false, A_stale = false;   // A_stale: tlpk_set_values* since the K2 copies were filled
        i64 asked[2] = {0, 0};                    // steps asked of the last call, per system
        i64 bytes = 0;                            // device memory of all of this (tlpk_symbolic_get "polish_bytes")
        int ipm_steps = 0;                        // tlpk_ipm_set_polish
    } polish;
    i64 mem_budget = 0;                           // tlpk_options.mem_budget_bytes (0 = none given): what a first-use allocation is held against
    int *h_info = nullptr;
    double *pin_in = nullptr, *pin_out = nullptr;   // pinned staging of the host-pointer entry points (lazily allocated)
    bool io_timing = false; double io_t_first = 0, io_t_last = 0;   // TLPK_HOSTIO_TIMING: when the first / last device-to-host group had landed
    std::vector<hipEvent_t> io_events;              // one per device-to-host piece of tlpk_solve (tlpk_api.cpp: stage_out)
    bool factored = false, local_done = false, solve_timed = false;
    enum class Pending { None, Solve, Pair, Refine } pending = Pending::None;   // which split-phase first half (tlpk_solve_local / tlpk_solve2_local / tlpk_refine_local) waits for its second
    i64 fail_col = -1;
    double ms_analyse = 0, ms_update = 0, ms_solve = 0;
    tlpk_kernel_times kt{};
    size_t factor_marker = 0, fwd_marker = 0;   // index of the LK_ALLREDUCE_ROOT launch (or size)
    i64 first_link = 0, nlink = 0;
    // persistent sweeps: ticket-counter slot of every sweep launch
    std::vector<i32> sweep_slot_fwd, sweep_slot_bwd;
    unsigned long long solve_epoch = 0;
    int poll[3] = {8, 16, 32};          // TLPK_POLL=fast,nfast,slow (tuning knob of the sweep kernels' polling back-off)
    // single-process multi-device mode (tlpk_create_multi): the parent owns one sharded handle per device
    std::vector<tlpk_handle *> sub;
    double *multi_tmp = nullptr;        // device 0: staging of the peers' root panels / root rhs for the reduction
    i64 multi_red_off = 0, multi_dy0_off = 0;   // ... followed by the reduced buffer and the lead's rank-local dy
    hipEvent_t multi_ev[MAX_DEVICES] = {}; hipEvent_t multi_done = nullptr;
    void *multi_comm[MAX_DEVICES] = {}; bool multi_rccl = false;   // TLPK_MULTI_REDUCE=rccl: one ncclComm_t per shard
    int multi_mode = 1;                 // parent: reduction of the root panel / rhs: 0 gather to the lead + broadcast, 1 reduce-scatter + all-gather over peer copies (default), 2 RCCL
    hipEvent_t multi_ev2[MAX_DEVICES] = {}; i64 rs_slice = 0;     // parent: 'slice broadcast' events, slice length (doubles) of the largest reduced buffer
    double *rs_stage = nullptr;         // child: staging of the peers' contributions to THIS shard's slice ((N - 1) x rs_slice doubles)
    void *shard_pool = nullptr;         // parent: one persistent host thread per shard (tlpk_api.cpp: ShardPool) -- the shards' launches are enqueued concurrently
    double ms_enqueue_update = 0;       // parent: host time from the entry of tlpk_update until every shard's work is enqueued
    i64 col_lo = 0, col_hi = 0, row_lo = 0, row_hi = 0, link_lo = 0, link_hi = 0;   // child: slices of the job-wide input vectors it reads
    bool stagger = false, stagger_armed = false; i64 stagger_min = 10000; hipEvent_t ev_stagger = nullptr;   // TLPK_STAGGER (experiment, tlpk_api.cpp: run_launches)
    // hipGraph replay of the static schedules (tlpk_api.cpp: graph_or_direct): instantiated graphs and their keys
    bool use_graph = true;              // TLPK_GRAPH=0 turns it off; switched off for good if capture fails on this system
    bool force_graph = false;           // TLPK_GRAPH=2: also for schedules with concurrent stream groups
    std::vector<hipGraphExec_t> graph_execs;
    std::vector<std::vector<char>> graph_keys;
    IpmState *ipm = nullptr;            // device-resident interior-point vectors (tlpk_ipm_load), freed by tlpk_destroy
    // tlpk_set_values: the maps from the caller's nzval to the value-dependent arrays (symbolic.cpp: build_value_maps), built and uploaded by the FIRST call
    ValueMaps vmaps;                    // host copy (analyse-only handles keep it; device handles drop the product maps once they are uploaded)
    i32 *d_pair_a = nullptr, *d_pair_b = nullptr, *d_ax_src = nullptr, *d_tx_src = nullptr, *d_px_src = nullptr;
    i64 n_px_src = 0;                   // entries of Px
    double *d_nz = nullptr;             // the caller's nzval on the device: d.Ax itself, or (K2: Ax holds the incidence matrix) a staging array
    bool values_set = false;            // tlpk_set_values* has run on this handle
    bool host_ax_stale = false;         // the last values came through a device pointer: S.Ax is copied back when a host consumer asks (sync_host_values)
    bool ipm_stale = false;             // new values since tlpk_ipm_load / tlpk_ipm_reload: the loops are refused until tlpk_ipm_reload
    i64 set_values_bytes = 0;           // device memory of the maps (tlpk_stats.set_values_bytes)
    double ms_set_values = 0;           // tlpk_stats.ms_last_set_values
    hipEvent_t sv_ev0 = nullptr, sv_ev1 = nullptr; bool sv_pending = false;   // ... of an enqueued refresh: read when the events have completed
    // matrix-free handles (tlpk_options.krylov; tlpk_api.cpp: krylov_*): no factor, an iteration per solve.  One of the three sets of arrays is in use:
    // conjugate gradients on K1 (krylov_kernels.hip), MINRES on K2 (krylov_k2_kernels.hip), TriCG on the quasi-definite form of K2 (krylov_sqd_kernels.hip)
    int krylov = 0, krylov_precond = 0;
    i64 krylov_itmax = 0; double krylov_atol = 0, krylov_rtol = 0;      // as resolved at create (0 -> 2 m, sqrt(eps))
    CgArrays cg;
    MrArrays mr;
    TcArrays tc;
    void *krylov_pin = nullptr;         // pinned copy of the method's scalar block, read after every chunk of iterations; behind sizeof(TcScalars): TriCG's update status word
    hipEvent_t krylov_ev = nullptr;
    i64 krylov_chunk0 = 4, krylov_chunk_max = 32;   // iterations enqueued before the first look at the outcome / at most between two looks (TLPK_CG_CHUNK=first,max)
    i64 krylov_iters = 0, krylov_iters_total = 0, krylov_converged = 0, krylov_launches = 0, krylov_unsolved = 0;
    double krylov_resid0 = 0, krylov_resid = 0;
    // tlpk_solve2_device on such a handle: both right-hand sides through one sequence of launches (tlpk_api.cpp: krylov_solve2).  The second set of vectors and
    // slots (cg2 / mr2 / tc2; its sc holds the TWO scalar blocks of a pair) and the pinned copy of both blocks are allocated by the first pair.  pair_state:
    // 0 = not tried, 1 = ready, -1 = the allocation failed or would cross the budget (every pair then runs as two solves and is counted in pair_fallbacks)
    bool krylov_pair_on = true;         // TLPK_KRYLOV_PAIR=0 at create: two ordinary solves, as before
    int krylov_pair_state = 0;
    double krylov_budget = 0;           // mem_budget_bytes (0 = none given)
    CgArrays cg2;
    MrArrays mr2;
    TcArrays tc2;
    void *krylov_pin2 = nullptr;
    i64 krylov_pairs = 0, krylov_pair_fallbacks = 0, krylov_pair_rounds = 0;      // paired solves / fallbacks since create; rounds enqueued by the last pair
    i64 krylov_pair_iters[2] = {0, 0}, krylov_pair_outcome[2] = {0, 0};          // of the last pair, per right-hand side (outcome: CG_SOLVED, CG_ITMAX, CG_BREAKDOWN)
    double krylov_pair_resid[4] = {0, 0, 0, 0};                                  // resid0, resid of number 0; resid0, resid of number 1
    // block skip (tlpk_block_skip / tlpk_ipm_batch_skip; tlpk_api.cpp: skip_*): units are the blocks of row_block, or the LPs of a batch-loaded handle
    std::vector<i32> front_unit;        // unit of every front, then of every single (the order of S.single_col); empty = not built yet
    i64 skip_units = 0;                 // number of units the table was built for
    bool skip_units_batch = false;      // ... and whether they are the LPs of the batch (tlpk_ipm_batch_skip) or the blocks of row_block (tlpk_block_skip)
    bool units_shared = false;          // the table holds fronts of unit `skip_units`: shared by several units, never skipped (tlpk_ipm_batch_factor_each's holds only)
    std::vector<unsigned char> skip_host;   // tlpk_block_skip: the bytes in force per front and then per single; empty = no mask
    i64 skip_dev_bytes = 0;             // device memory of the tables (tlpk_symbolic_get "skip_bytes")
    bool batch_skip = false;            // tlpk_ipm_batch_skip(h, 1)
    std::string last_error;
};
// tlpk_api.cpp, block skip.  skip_build_units: the front_unit table from the unit of every row and column of the caller's A (a column's unit is only read for
// K2), verified -- TLPK_BADARG with a sentence and nothing changed if a front is not contained in one unit.  skip_device_tables: the device copies, once.
// skip_from_flags: the mask of the NEXT update / solves from per-unit flags in device memory (flag[k * stride] == 0.0 -> unit k is skipped), enqueued on the
// handle's stream; skip_off: no mask (the tables stay)
// allow_shared: a front whose columns lie in several units is accepted, with unit `nunits` (one behind the last: the caller's flags never skip it), if it stands alone -- no rows below its pivot block and no
// children, so that it neither feeds nor is fed by a front that a mask leaves out (K2: the root front of the columns of A without entries)
int skip_build_units(tlpk_handle *h, const std::vector<i32> &row_unit, const std::vector<i32> &col_unit, i64 nunits, const char *what, bool allow_shared = false);
int skip_device_tables(tlpk_handle *h);
int skip_from_flags(tlpk_handle *h, const double *d_flag, int stride);
void skip_off(tlpk_handle *h);

void ipm_free(tlpk_handle *h);          // tlpk_ipm.cpp
bool ipm_is_batch(const tlpk_handle *h);   // tlpk_ipm.cpp: the handle holds a stack of LPs (tlpk_ipm_load_batch)
// tlpk_ipm.cpp, for the refinement on demand of a K2 handle (whose own arrays hold the incidence matrix): the host copies of A, column-major and
// row-major, as the loops build theirs; the loops' own device copies of the whole A (false: none -- no LP loaded, a stack of LPs, or the loops share the handle's)
int ipm_host_matrix(tlpk_handle *h, std::vector<i64> &ap, std::vector<i32> &ai, std::vector<double> &ax, std::vector<i64> &tp, std::vector<i32> &tj, std::vector<double> &tx);
bool ipm_matrix(const tlpk_handle *h, PolishMat &A);
int sync_host_values(tlpk_handle *h);   // tlpk_api.cpp: S.Ax <- the device copy after a tlpk_set_values*_device
// tlpk_api.cpp, for tlpk_ipm_batch_refill: the refresh of tlpk_set_values restricted to the LPs of a stack whose flag is set (d_flag[k * stride] != 0; d_lp_of: the LP of
// every entry of nzval; ranges: (lo, hi) pairs, the entries of nzval that are read).  Enqueued on the handle's stream.
int set_values_slots(tlpk_handle *h, const double *nzval, const std::vector<i64> &ranges, const i32 *d_lp_of, const double *d_flag, int stride);
// tlpk_api.cpp, for the device-resident interior-point loops on a multi-device handle: KKT.update! from the theta / regP / regD every
// shard holds on its device, and KKT.solve! with shard-resident vectors in the rank-local layout (every shard adds ITS xi_p on the
// linking rows -- partial residuals --, the library's reduction completes them; nothing is gathered)
int multi_update_resident(tlpk_handle *h);
int multi_solve_resident(tlpk_handle *h, double *const *dx, double *const *dy, const double *const *xip, const double *const *xid);
int multi_solve2_resident(tlpk_handle *h, double *const *dx0, double *const *dy0, const double *const *xip0, const double *const *xid0,
                          double *const *dx1, double *const *dy1, const double *const *xip1, const double *const *xid1);



inline int hip_fail(tlpk_handle *h, hipError_t e, const char *what) {
    h->last_error = std::string(what) + ": " + hipGetErrorString(e);
    return (e == hipErrorOutOfMemory) ? TLPK_OOM : TLPK_HIPERR;
}
#ifndef HIPCHK
#define HIPCHK(h, call)                                                   \
    do {                                                                  \
        hipError_t e_ = (call);                                           \
        if (e_ != hipSuccess) return hip_fail((h), e_, #call);            \
    } while (0)
#endif

template <class T>
inline int dev_alloc(tlpk_handle *h, T **out, i64 count) {
    *out = nullptr;
    const size_t bytes = (size_t)std::max<i64>(count, 1) * sizeof(T);
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return hip_fail(h, e, "hipMalloc");
    h->allocs.push_back(p);
    h->device_bytes += (i64)bytes;
    *out = (T *)p;
    return TLPK_OK;
}
template <class T, class A>
inline int dev_upload(tlpk_handle *h, T **out, const std::vector<T, A> &v) {
    int rc = dev_alloc(h, out, (i64)v.size());
    if (rc != TLPK_OK) return rc;
    if (!v.empty()) HIPCHK(h, hipMemcpy(*out, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return TLPK_OK;
}

