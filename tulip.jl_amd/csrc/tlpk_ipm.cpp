// tlpk_ipm.cpp -- C ABI of the device-resident interior-point vectors (include/tlpk.h, section
// "Device-resident HSD iterate").
//
// With the drop-in KKT interface (tlpk_update / tlpk_solve) every solve moves 16 (m + n) bytes over
// PCIe and the host builds every right-hand side.  Here the iterate, the residuals, the right-hand
// sides and the search directions of Tulip's homogeneous self-dual loop live in HBM; a call runs one
// routine of /root/reference/src/IPM/HSD/{HSD.jl, step.jl} on the device and returns the handful of
// scalars the host logic needs (norms, dot products, step lengths).  The host keeps tau, kappa, the
// regularisation scalars and the control flow (tulip.jl_amd/hsd_device.py mirrors HSD.jl:203-350).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "tlpk_handle.hpp"
#include "tlpk_ipm.hpp"

struct IpmState {
    IpmVecs v{};
    IpmDir D[2]{};                  // D[cur] = accepted direction, D[1 - cur] = candidate of the centrality corrector
    int cur = 0;
    double *partials[2] = {nullptr, nullptr};     // per-block partial results of two concurrent reductions
    double *d_out = nullptr;        // finalised scalars on the device
    double *h_out = nullptr;        // ... and in pinned host memory
    int pre_blocks = 0;
    // multi-device parent only: the linking rows (user indices, ascending), b on them, staging for the shards' partial rp
    std::vector<i64> link_rows; std::vector<double> b_link; double *h_link = nullptr; i64 link_lo = 0, link_hi = 0;
    struct IpmBatchState *bat = nullptr;      // tlpk_ipm_load_batch: the handle holds a stack of LPs (the tlpk_ipm_batch_* calls serve it)
};

// a stack of LPs on one single-device handle: segment offsets, the block tables of ipm_batch_kernels.hip and buffers sized by the number of LPs
struct IpmBatchState {
    i64 nlp = 0;
    std::vector<i64> row_off, col_off;
    IpmBatch B{};
    double *partials[2] = {nullptr, nullptr};     // rows = blocks of the longest table
    double *d_out = nullptr, *h_out = nullptr;    // 2 x nlp x IPM_SLOTS finalised scalars (device / pinned)
    double *d_sc = nullptr, *h_sc = nullptr;      // nlp x IPM_BSC scalars of the current call (device / pinned)
    double *sx[2] = {nullptr, nullptr}, *sy[2] = {nullptr, nullptr};      // what the solves write (n, m; two right-hand sides): the active LPs take their segments from here
    // tlpk_ipm_batch_refill, built by its first call that brings new values: the LPs' contiguous ranges of the caller's nzval, the LP of every entry of it and -- K2,
    // whose loops keep their own copies of A -- for every entry of the row-major copy the position in nzval it copies
    bool refill_maps = false;
    std::vector<i64> nz_off;
    i32 *d_lp_of = nullptr, *d_ktx_src = nullptr;
    // tlpk_ipm_get_lps, allocated by its first call and grown by a later, larger one: the device staging of the gathered segments and the segment table (device / pinned)
    double *d_stage = nullptr; i64 stage_cap = 0;
    IpmGatherSeg *d_tab = nullptr, *h_tab = nullptr; i64 tab_cap = 0;
    // tlpk_ipm_batch_factor_each, allocated by its first call with the device tables (DevArrays.fail_words ...): the pinned copy of the per-LP verdicts
    int *h_fail = nullptr;
};

// ---- one device or several ---------------------------------------------------------------------------------------------------
// On a tlpk_create_multi handle (block-angular LP; K1, or K2 -- then the variable nodes of the replicated root front count as the
// lead shard's columns) every shard holds the SUB-LP of its diagonal blocks in vectors of the job's
// full length: its own columns with their costs and bounds (the other columns are empty: cost 0, no bounds, no entries of A), its
// block rows of b, and the linking rows -- b on the lead shard only, A restricted to the shard's columns.  Every kernel of
// ipm_kernels.hip then computes, unchanged, the shard's share of each sum / maximum / minimum (an empty column or row contributes
// the neutral element), the host combines the shards' scalars in shard order, and three things cross the shards:
//   * the KKT solves: split-phase, EVERY shard adds its xi_p on the linking rows (its partial residual; b only on the lead), the
//     library's reduction of the root right-hand side completes the rows; solutions stay shard-resident (own columns / block
//     rows, linking rows replicated -- y, dy on them are updated identically everywhere);
//   * the factorisation: the usual reduction of the root panel;
//   * |rp|inf and |A x|inf on the linking rows (tlpk_ipm_residuals): the shards' partial rp of those rows are summed on the host.
// A single-device handle is the same code with one shard.
namespace {

struct Shards { tlpk_handle *c[MAX_DEVICES]; int n = 0; bool multi = false; };

int ipm_shards(tlpk_handle *h, Shards &sh, bool need_loaded = true, bool allow_stale = false, bool allow_batch = false) {
    if (!h) return TLPK_BADARG;
    if (!h->has_device) return TLPK_NO_DEVICE;
    if (h->opt.nranks > 1) { h->last_error = "the device-resident IPM vectors need a single-rank or a tlpk_create_multi handle (a sharded handle's reductions belong to its caller)"; return TLPK_BADARG; }
    if (!h->sub.empty()) {
        sh.multi = true; sh.n = (int)h->sub.size();
        for (int r = 0; r < sh.n; ++r) sh.c[r] = h->sub[(size_t)r];
    } else { sh.multi = false; sh.n = 1; sh.c[0] = h; }
    if (need_loaded && !h->ipm) { h->last_error = "tlpk_ipm_load has not been called"; return TLPK_BADARG; }
    if (need_loaded && h->ipm->bat && !allow_batch) {
        h->last_error = "the handle holds a stack of LPs (tlpk_ipm_load_batch): use the tlpk_ipm_batch_* calls (tlpk_ipm_reset, tlpk_ipm_reload and tlpk_ipm_get are shared)";
        return TLPK_BADARG;
    }
    if (need_loaded && h->ipm_stale && !allow_stale) {
        h->last_error = "the matrix values changed (tlpk_set_values) after the LP was loaded: call tlpk_ipm_reload before the device-resident loops";
        return TLPK_BADARG;
    }
    return TLPK_OK;
}
int fail_from(tlpk_handle *h, tlpk_handle *c, int rc) { if (c != h) h->last_error = c->last_error; return rc; }

// after every shard has finalised `count` scalars at d_out: copy them to the host, wait, combine in shard order
// (slots [0, nsum) sums, then nmax maxima, then nmin minima) into res
int gather(tlpk_handle *h, Shards &sh, int count, int nsum, int nmax, double *res) {
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r]; IpmState &s = *c->ipm;
        HIPCHK(h, hipSetDevice(c->device));
        HIPCHK(h, hipMemcpyAsync(s.h_out, s.d_out, (size_t)count * 8, hipMemcpyDeviceToHost, c->stream));
    }
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r];
        HIPCHK(h, hipSetDevice(c->device));
        HIPCHK(h, hipStreamSynchronize(c->stream));
        HIPCHK(h, hipGetLastError());
    }
    for (int k = 0; k < count; ++k) {
        double v = sh.c[0]->ipm->h_out[k];
        for (int r = 1; r < sh.n; ++r) {
            const double w = sh.c[r]->ipm->h_out[k];
            v = (k < nsum) ? v + w : (k < nsum + nmax ? std::fmax(v, w) : std::fmin(v, w));
        }
        res[k] = v;
    }
    return TLPK_OK;
}
// slots laid out in two groups of IPM_SLOTS (two concurrent reductions): group g has its own (nsum, nmax)
int gather2(tlpk_handle *h, Shards &sh, int nsum0, int nmax0, int cnt0, int nsum1, int nmax1, int cnt1, double *res) {
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r]; IpmState &s = *c->ipm;
        HIPCHK(h, hipSetDevice(c->device));
        HIPCHK(h, hipMemcpyAsync(s.h_out, s.d_out, (size_t)(IPM_SLOTS + cnt1) * 8, hipMemcpyDeviceToHost, c->stream));
    }
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r];
        HIPCHK(h, hipSetDevice(c->device));
        HIPCHK(h, hipStreamSynchronize(c->stream));
        HIPCHK(h, hipGetLastError());
    }
    for (int g = 0; g < 2; ++g) {
        const int off = g * IPM_SLOTS, cnt = g ? cnt1 : cnt0, ns = g ? nsum1 : nsum0, nm = g ? nmax1 : nmax0;
        for (int k = 0; k < cnt; ++k) {
            double v = sh.c[0]->ipm->h_out[off + k];
            for (int r = 1; r < sh.n; ++r) {
                const double w = sh.c[r]->ipm->h_out[off + k];
                v = (k < ns) ? v + w : (k < ns + nm ? std::fmax(v, w) : std::fmin(v, w));
            }
            res[off + k] = v;
        }
    }
    return TLPK_OK;
}
int sync_all(tlpk_handle *h, Shards &sh) {
    for (int r = 0; r < sh.n; ++r) { const int rc = tlpk_sync(sh.c[r]); if (rc != TLPK_OK) return fail_from(h, sh.c[r], rc); }
    return TLPK_OK;
}
// KKT.update! with the theta / regularisation vectors every shard has just written
int update_all(tlpk_handle *h, Shards &sh) {
    if (!sh.multi) return tlpk_update_device(h, h->d_theta, h->d_regP, h->d_regD);
    return multi_update_resident(h);
}
// KKT.solve! per shard: pick(state) -> {dx, dy, xi_p, xi_d}
template <class F>
int solve_all(tlpk_handle *h, Shards &sh, F &&pick) {
    double *dx[MAX_DEVICES], *dy[MAX_DEVICES]; const double *xp[MAX_DEVICES], *xd[MAX_DEVICES];
    for (int r = 0; r < sh.n; ++r) pick(*sh.c[r]->ipm, dx[r], dy[r], xp[r], xd[r]);
    if (!sh.multi) {
        const int rc = tlpk_solve_device(h, dx[0], dy[0], xp[0], xd[0]);
        // tlpk_ipm_set_polish: every KKT solve of the loops is followed by guarded refinement steps on the same vectors
        return rc != TLPK_OK || h->polish.ipm_steps == 0 ? rc : tlpk_polish_device(h, dx[0], dy[0], xp[0], xd[0], h->polish.ipm_steps);
    }
    return multi_solve_resident(h, dx, dy, xp, xd);
}

}  // namespace

// dense-matrix handle: A'y and / or A x of the current iterate into the vectors the residual kernels read
static void dense_products(tlpk_handle *c, bool cols, bool rows) {
    if (!c->S.dense_matrix) return;
    const IpmVecs &v = c->ipm->v;
    if (cols) { const double *y[1] = {v.y}, *none[1] = {nullptr}; double *o[1] = {const_cast<double *>(v.aty)}; launch_dense_gemv_t(c->stream, c->d, nullptr, y, none, o, 1); }
    if (rows) { const double *x[1] = {v.x}, *none[1] = {nullptr}; double *o[1] = {const_cast<double *>(v.ax)}; launch_dense_gemv_n(c->stream, c->d, nullptr, x, none, o, 1); }
}

bool ipm_is_batch(const tlpk_handle *h) { return h && h->ipm && h->ipm->bat; }
void ipm_free(tlpk_handle *h) {
    if (!h || !h->ipm) return;
    if (h->ipm->h_out) hipHostFree(h->ipm->h_out);
    if (h->ipm->h_link) hipHostFree(h->ipm->h_link);
    if (IpmBatchState *bs = h->ipm->bat) {
        if (bs->h_out) hipHostFree(bs->h_out);
        if (bs->h_sc) hipHostFree(bs->h_sc);
        if (bs->h_tab) hipHostFree(bs->h_tab);
        if (bs->h_fail) hipHostFree(bs->h_fail);
        if (bs->d_tab) hipFree(bs->d_tab);
        if (bs->d_stage) hipFree(bs->d_stage);
        delete bs;
    }
    delete h->ipm;                  // device vectors are in h->allocs
    h->ipm = nullptr;
}

extern "C" {

// mask = nullptr: the whole LP on handle c (a single-device handle).  Otherwise c is a shard of a multi-device handle and takes the
// sub-LP of the columns / rows it owns (see the comment at the top).
static int ipm_load_impl(tlpk_handle *h, const double *b, const double *c, const double *l, const double *u, bool shard);

int tlpk_ipm_load(tlpk_handle *h, const double *b, const double *c, const double *l, const double *u) {
    // a failed load leaves no half-initialised state behind: later tlpk_ipm_* calls report "not loaded", a retry is possible
    Shards sh;
    if (int rc = ipm_shards(h, sh, false)) return rc;
    if (!b || !c || !l || !u) return TLPK_BADARG;
    if (h->ipm) { h->last_error = "tlpk_ipm_load called twice on one handle"; return TLPK_BADARG; }
    int rc = TLPK_OK;
    if (!sh.multi) rc = ipm_load_impl(h, b, c, l, u, false);
    else {
        for (int r = 0; r < sh.n && rc == TLPK_OK; ++r) {
            rc = ipm_load_impl(sh.c[r], b, c, l, u, true);
            if (rc != TLPK_OK) h->last_error = sh.c[r]->last_error;
        }
        if (rc == TLPK_OK) {
            IpmState *sp = new (std::nothrow) IpmState();           // the parent's state: what the host needs for the linking rows
            if (!sp) rc = TLPK_OOM;
            else {
                h->ipm = sp;
                const Symbolic &S0 = sh.c[0]->S;
                const bool k2 = S0.system == 1;
                const i64 mm = k2 ? S0.k2_m : S0.m, off = k2 ? S0.k2_n : 0;
                for (i64 i = 0; i < mm; ++i) if (S0.row_local[(size_t)(off + i)] == 2) { sp->link_rows.push_back(i); sp->b_link.push_back(b[i]); }
                if (!sp->link_rows.empty()) {
                    sp->link_lo = sp->link_rows.front(); sp->link_hi = sp->link_rows.back() + 1;
                    if (hipHostMalloc((void **)&sp->h_link, (size_t)(sp->link_hi - sp->link_lo) * (size_t)sh.n * 8, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); rc = TLPK_OOM; }
                }
            }
        }
    }
    if (rc != TLPK_OK) { ipm_free(h); if (sh.multi) for (int r = 0; r < sh.n; ++r) ipm_free(sh.c[r]); }
    return rc;
}

// The copy of A the loops of handle h read where they cannot share the handle's own (a shard's sub-LP; K2, whose handle holds the incidence matrix of the
// augmented system): host copy of A, column-major: K1 -- the analyse phase's copy; K2 -- rebuilt from the incidence matrix
// (column p = entry p of A: 1 on variable node j, A[i,j] on constraint node n + i, in A's column-major entry order).
// A shard keeps the columns it owns (the others are empty).  Then the row-major copy.  tlpk_ipm_load uploads all six arrays, tlpk_ipm_reload the two value arrays.
static int ipm_sub_matrix(tlpk_handle *h, bool shard, std::vector<i64> &ap, std::vector<i32> &ai, std::vector<double> &ax,
                          std::vector<i64> &tp, std::vector<i32> &tj, std::vector<double> &tx) {
    if (int rc = sync_host_values(h)) return rc;
    const Symbolic &S = h->S;
    const bool k2 = S.system == 1;
    const i64 m = k2 ? S.k2_m : S.m - S.n_dense, n = k2 ? S.k2_n : S.n;
    auto own_col = [&](i64 j) { if (!shard) return true; if (!k2) return S.col_local[(size_t)j] != 0; const char nl = S.row_local[(size_t)j]; return nl == 1 || (nl == 2 && h->opt.rank == 0); };
    ap.assign((size_t)n + 1, 0); tp.assign((size_t)m + 1, 0);
    ai.clear(); tj.clear(); ax.clear(); tx.clear();
    if (!k2) {
        for (i64 j = 0; j < n; ++j) {
            if (own_col(j)) for (i64 q = S.Ap[(size_t)j]; q < S.Ap[(size_t)j + 1]; ++q) { ai.push_back(S.Ai[(size_t)q]); ax.push_back(S.Ax[(size_t)q]); }
            ap[(size_t)j + 1] = (i64)ai.size();
        }
    } else {
        const i64 nnz = S.n;
        i64 jprev = 0;
        for (i64 p = 0; p < nnz; ++p) {
            if (S.Ap[(size_t)p + 1] - S.Ap[(size_t)p] != 2) { h->last_error = "K2 incidence matrix: unexpected column"; return TLPK_INTERNAL; }
            const i64 q = S.Ap[(size_t)p];
            const i32 a = S.Ai[(size_t)q], b2 = S.Ai[(size_t)q + 1];
            const bool afirst = a < (i32)n;                   // the variable node is the smaller index
            const i64 j = afirst ? a : b2; const i32 i = (afirst ? b2 : a) - (i32)n;
            if (j < jprev) { h->last_error = "K2 incidence matrix: columns out of order"; return TLPK_INTERNAL; }
            for (; jprev < j; ++jprev) ap[(size_t)jprev + 1] = (i64)ai.size();
            if (own_col(j)) { ai.push_back(i); ax.push_back(S.Ax[(size_t)q + (afirst ? 1 : 0)]); }
        }
        for (; jprev < n; ++jprev) ap[(size_t)jprev + 1] = (i64)ai.size();
    }
    for (size_t q = 0; q < ai.size(); ++q) ++tp[(size_t)ai[q] + 1];
    for (i64 i = 0; i < m; ++i) tp[(size_t)i + 1] += tp[(size_t)i];
    tj.resize(ai.size()); tx.resize(ai.size());
    { std::vector<i64> cur(tp.begin(), tp.end() - 1);
      for (i64 j = 0; j < n; ++j) for (i64 q = ap[(size_t)j]; q < ap[(size_t)j + 1]; ++q) { const i64 c2 = cur[(size_t)ai[(size_t)q]]++; tj[(size_t)c2] = (i32)j; tx[(size_t)c2] = ax[(size_t)q]; } }
    return TLPK_OK;
}
extern "C++" int ipm_host_matrix(tlpk_handle *h, std::vector<i64> &ap, std::vector<i32> &ai, std::vector<double> &ax, std::vector<i64> &tp, std::vector<i32> &tj,
                                 std::vector<double> &tx) {
    return ipm_sub_matrix(h, false, ap, ai, ax, tp, tj, tx);
}
extern "C++" bool ipm_matrix(const tlpk_handle *h, PolishMat &A) {
    if (!h->ipm || h->ipm->bat || h->S.dense_matrix) return false;
    const IpmVecs &v = h->ipm->v;
    if (v.Ap == h->d.Ap || !v.Ap) return false;
    A = PolishMat{v.m, v.n, v.Ap, v.Ai, v.Ax, v.Tp, v.Tj, v.Tx};
    return true;
}

static int ipm_load_impl(tlpk_handle *h, const double *b, const double *c, const double *l, const double *u, bool shard) {
    HIPCHK(h, hipSetDevice(h->device));
    const bool k2 = h->S.system == 1;
    const i64 m = k2 ? h->S.k2_m : h->S.m - h->S.n_dense, n = k2 ? h->S.k2_n : h->S.n;      // (dense columns: S.m is the order m + k of the factored matrix)
    IpmState *sp = new (std::nothrow) IpmState();
    if (!sp) return TLPK_OOM;
    h->ipm = sp;
    IpmState &s = *sp;
    IpmVecs &v = s.v;
    v.m = m; v.n = n; v.row_skip = nullptr; v.aty = nullptr; v.ax = nullptr;
    int rc;
    const Symbolic &S = h->S;
    // ownership of columns (variables) and rows (constraints) on a shard: K1 -- the column / row maps of the analyse phase; K2 -- the
    // node map (variable nodes 0 .. n-1, constraint nodes n .. n+m-1): a node of the replicated root front belongs to the lead shard
    auto own_col = [&](i64 j) { if (!shard) return true; if (!k2) return S.col_local[(size_t)j] != 0; const char nl = S.row_local[(size_t)j]; return nl == 1 || (nl == 2 && h->opt.rank == 0); };
    auto row_kind = [&](i64 i) -> char { return k2 ? S.row_local[(size_t)(n + i)] : S.row_local[(size_t)i]; };      // 0 other shard, 1 own, 2 linking (replicated)
    if (h->S.dense_matrix) {
        // no index arrays for a dense A (they would cost 12 m n bytes beside the 8 m n of A): the kernels read A'y and A x from two vectors
        // that dense_products() fills with the GEMV kernels of the solves
        double *p1, *p2;
        if ((rc = dev_alloc(h, &p1, n)) != TLPK_OK) return rc;
        if ((rc = dev_alloc(h, &p2, m)) != TLPK_OK) return rc;
        v.aty = p1; v.ax = p2;
    } else if (!shard && !k2) { v.Ap = h->d.Ap; v.Ai = h->d.Ai; v.Ax = h->d.Ax; v.Tp = h->d.Tp; v.Tj = h->d.Tj; v.Tx = h->d.Tx; }
    else {
        // host copy of A, column-major: K1 -- the analyse phase's copy; K2 -- rebuilt from the incidence matrix of the augmented system
        // it holds (column p = entry p of A: 1 on variable node j, A[i,j] on constraint node n + i, in A's column-major entry order).
        // A shard keeps the columns it owns (the others are empty).  Then the row-major copy.
        std::vector<i64> ap, tp; std::vector<i32> ai, tj; std::vector<double> ax, tx;
        if ((rc = ipm_sub_matrix(h, shard, ap, ai, ax, tp, tj, tx)) != TLPK_OK) return rc;
        i64 *dp; i32 *di; double *dxv;
        if ((rc = dev_upload(h, &dp, ap)) != TLPK_OK) return rc; v.Ap = dp;
        if ((rc = dev_upload(h, &di, ai)) != TLPK_OK) return rc; v.Ai = di;
        if ((rc = dev_upload(h, &dxv, ax)) != TLPK_OK) return rc; v.Ax = dxv;
        if ((rc = dev_upload(h, &dp, tp)) != TLPK_OK) return rc; v.Tp = dp;
        if ((rc = dev_upload(h, &di, tj)) != TLPK_OK) return rc; v.Tj = di;
        if ((rc = dev_upload(h, &dxv, tx)) != TLPK_OK) return rc; v.Tx = dxv;
        if (shard) {
            char *dc;
            std::vector<char> skip((size_t)m);
            for (i64 i = 0; i < m; ++i) skip[(size_t)i] = row_kind(i) == 2;      // linking rows: partial sums, no part in the maxima
            if ((rc = dev_upload(h, &dc, skip)) != TLPK_OK) return rc; v.row_skip = dc;
        }
    }
    // problem data: b, c, l .* lflag, u .* uflag, flags (ipmdata.jl:46-47); a shard: its sub-LP
    std::vector<double> lz((size_t)n), uz((size_t)n), lf((size_t)n), uf((size_t)n), bb, cc;
    for (i64 j = 0; j < n; ++j) {
        const bool own = own_col(j);
        const bool fl = own && std::isfinite(l[j]), fu = own && std::isfinite(u[j]);
        lf[(size_t)j] = fl ? 1.0 : 0.0; uf[(size_t)j] = fu ? 1.0 : 0.0;
        lz[(size_t)j] = fl ? l[j] : 0.0; uz[(size_t)j] = fu ? u[j] : 0.0;
    }
    if (shard) {
        bb.assign((size_t)m, 0.0); cc.assign((size_t)n, 0.0);
        for (i64 i = 0; i < m; ++i) { const char rl = row_kind(i); if (rl == 1 || (rl == 2 && h->opt.rank == 0)) bb[(size_t)i] = b[i]; }
        for (i64 j = 0; j < n; ++j) if (own_col(j)) cc[(size_t)j] = c[j];
        b = bb.data(); c = cc.data();
    }
    double *p;
#define UPV(dst, ptr, len) do { if ((rc = dev_alloc(h, &p, (len))) != TLPK_OK) return rc; if ((len) > 0) HIPCHK(h, hipMemcpy(p, (ptr), (size_t)(len) * 8, hipMemcpyHostToDevice)); dst = p; } while (0)
    UPV(v.b, b, m); UPV(v.c, c, n); UPV(v.lz, lz.data(), n); UPV(v.uz, uz.data(), n); UPV(v.lflag, lf.data(), n); UPV(v.uflag, uf.data(), n);
#undef UPV
#define ALV(dst, len) do { if ((rc = dev_alloc(h, &p, (len))) != TLPK_OK) return rc; HIPCHK(h, hipMemset(p, 0, (size_t)std::max<i64>((len), 1) * 8)); dst = p; } while (0)
    ALV(v.x, n); ALV(v.xl, n); ALV(v.xu, n); ALV(v.zl, n); ALV(v.zu, n); ALV(v.y, m);
    ALV(v.rp, m); ALV(v.rl, n); ALV(v.ru, n); ALV(v.rd, n); ALV(v.thl, n); ALV(v.thu, n); ALV(v.hx, n); ALV(v.hy, m); ALV(v.hxid, n);
    ALV(v.xil, n); ALV(v.xiu, n); ALV(v.xzl, n); ALV(v.xzu, n); ALV(v.xid, n); ALV(v.xip, m);
    for (int k = 0; k < 2; ++k) { ALV(s.D[k].x, n); ALV(s.D[k].xl, n); ALV(s.D[k].xu, n); ALV(s.D[k].zl, n); ALV(s.D[k].zu, n); ALV(s.D[k].y, m); }
    ALV(s.partials[0], (i64)IPM_BLOCKS * IPM_SLOTS); ALV(s.partials[1], (i64)IPM_BLOCKS * IPM_SLOTS);
    ALV(s.d_out, 2 * IPM_SLOTS);
#undef ALV
    HIPCHK(h, hipHostMalloc((void **)&s.h_out, 2 * IPM_SLOTS * sizeof(double), hipHostMallocDefault));
    ipm_launch_init(h->stream, v);                                       // HSD.jl:238-247
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    return TLPK_OK;
}

// tlpk_ipm_reload on one handle (shard = a shard of a multi-device handle: its sub-LP).  Everything is written into the vectors tlpk_ipm_load allocated.
static int ipm_reload_impl(tlpk_handle *h, const double *b, const double *c, const double *l, const double *u, bool shard) {
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));              // nothing of the previous run reads the vectors any more
    IpmState &s = *h->ipm;
    IpmVecs &v = s.v;
    const Symbolic &S = h->S;
    const bool k2 = S.system == 1;
    const i64 m = v.m, n = v.n;
    auto own_col = [&](i64 j) { if (!shard) return true; if (!k2) return S.col_local[(size_t)j] != 0; const char nl = S.row_local[(size_t)j]; return nl == 1 || (nl == 2 && h->opt.rank == 0); };
    auto row_kind = [&](i64 i) -> char { return k2 ? S.row_local[(size_t)(n + i)] : S.row_local[(size_t)i]; };
    if (!S.dense_matrix && (shard || k2)) {
        // the loops' own copy of A: same pattern, new values, in place
        std::vector<i64> ap, tp; std::vector<i32> ai, tj; std::vector<double> ax, tx;
        if (int rc = ipm_sub_matrix(h, shard, ap, ai, ax, tp, tj, tx)) return rc;
        if (!ax.empty()) {
            HIPCHK(h, hipMemcpy(const_cast<double *>(v.Ax), ax.data(), ax.size() * 8, hipMemcpyHostToDevice));
            HIPCHK(h, hipMemcpy(const_cast<double *>(v.Tx), tx.data(), tx.size() * 8, hipMemcpyHostToDevice));
        }
    }
    std::vector<double> w0, w1;
    auto put = [&](const double *dst, const std::vector<double> &src) -> int {
        if (!src.empty()) HIPCHK(h, hipMemcpy(const_cast<double *>(dst), src.data(), src.size() * 8, hipMemcpyHostToDevice));
        return TLPK_OK;
    };
    if (b) {
        w0.assign((size_t)m, 0.0);
        for (i64 i = 0; i < m; ++i) { const char rl = shard ? row_kind(i) : 1; if (rl == 1 || (rl == 2 && h->opt.rank == 0)) w0[(size_t)i] = b[i]; }
        if (int rc = put(v.b, w0)) return rc;
    }
    if (c) {
        w0.assign((size_t)n, 0.0);
        for (i64 j = 0; j < n; ++j) if (own_col(j)) w0[(size_t)j] = c[j];
        if (int rc = put(v.c, w0)) return rc;
    }
    for (int side = 0; side < 2; ++side) {
        const double *bd = side ? u : l;
        if (!bd) continue;
        w0.assign((size_t)n, 0.0); w1.assign((size_t)n, 0.0);          // flag, bound .* flag (ipmdata.jl:46-47)
        for (i64 j = 0; j < n; ++j) if (own_col(j) && std::isfinite(bd[j])) { w0[(size_t)j] = 1.0; w1[(size_t)j] = bd[j]; }
        if (int rc = put(side ? v.uflag : v.lflag, w0)) return rc;
        if (int rc = put(side ? v.uz : v.lz, w1)) return rc;
    }
    // the state of a fresh load: every work vector zero, then the starting point (HSD.jl:238-247)
    double *nv[] = {v.x, v.xl, v.xu, v.zl, v.zu, v.rl, v.ru, v.rd, v.thl, v.thu, v.hx, v.hxid, v.xil, v.xiu, v.xzl, v.xzu, v.xid,
                    s.D[0].x, s.D[0].xl, s.D[0].xu, s.D[0].zl, s.D[0].zu, s.D[1].x, s.D[1].xl, s.D[1].xu, s.D[1].zl, s.D[1].zu};
    double *mv[] = {v.y, v.rp, v.hy, v.xip, s.D[0].y, s.D[1].y};
    for (double *p : nv) HIPCHK(h, hipMemsetAsync(p, 0, (size_t)std::max<i64>(n, 1) * 8, h->stream));
    for (double *p : mv) HIPCHK(h, hipMemsetAsync(p, 0, (size_t)std::max<i64>(m, 1) * 8, h->stream));
    HIPCHK(h, hipMemsetAsync(s.partials[0], 0, (size_t)IPM_BLOCKS * IPM_SLOTS * 8, h->stream));
    HIPCHK(h, hipMemsetAsync(s.partials[1], 0, (size_t)IPM_BLOCKS * IPM_SLOTS * 8, h->stream));
    HIPCHK(h, hipMemsetAsync(s.d_out, 0, 2 * IPM_SLOTS * 8, h->stream));
    s.cur = 0;
    ipm_launch_init(h->stream, v);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    return TLPK_OK;
}

int tlpk_ipm_reload(tlpk_handle *h, const double *b, const double *c, const double *l, const double *u) {
    Shards sh;
    if (int rc = ipm_shards(h, sh, false)) return rc;
    if (!h->ipm) { h->last_error = "tlpk_ipm_reload: no LP is loaded on this handle (call tlpk_ipm_load first)"; return TLPK_BADARG; }
    int rc = TLPK_OK;
    if (!sh.multi) rc = ipm_reload_impl(h, b, c, l, u, false);
    else {
        for (int r = 0; r < sh.n && rc == TLPK_OK; ++r) {
            rc = ipm_reload_impl(sh.c[r], b, c, l, u, true);
            if (rc != TLPK_OK) h->last_error = sh.c[r]->last_error;
        }
        if (rc == TLPK_OK && b) { IpmState &ps = *h->ipm; for (size_t k = 0; k < ps.link_rows.size(); ++k) ps.b_link[k] = b[ps.link_rows[k]]; }
    }
    if (rc == TLPK_OK) h->ipm_stale = false;
    return rc;
}

int tlpk_ipm_reset(tlpk_handle *h) {
    Shards sh;
    if (int rc = ipm_shards(h, sh, true, false, true)) return rc;
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r];
        HIPCHK(h, hipSetDevice(c->device));
        ipm_launch_init(c->stream, c->ipm->v);
    }
    return TLPK_OK;
}

/* From now on every KKT solve of the unbatched loops on this handle is followed by `steps` guarded refinement steps (tlpk_polish_device; the pair of
 * tlpk_ipm_hsolve_newton by tlpk_polish2_device).  steps = 0: the calls as they are without it. */
int tlpk_ipm_set_polish(tlpk_handle *h, int steps) {
    if (!h) return TLPK_BADARG;
    const char *kind = !h->sub.empty() ? "a multi-device handle" : h->opt.nranks > 1 ? "a sharded handle" : h->S.dense_matrix ? "a dense-matrix handle"
                     : h->krylov ? "a matrix-free handle" : ipm_is_batch(h) ? "a batch-loaded handle" : nullptr;
    if (kind) { h->last_error = std::string("tlpk_ipm_set_polish: single-device handles with a factor and one LP loaded only; this is ") + kind; return TLPK_BADARG; }
    if (!h->has_device) return TLPK_NO_DEVICE;
    if (!h->ipm) { h->last_error = "tlpk_ipm_set_polish: tlpk_ipm_load has not been called"; return TLPK_BADARG; }
    if (steps < 0) { h->last_error = "tlpk_ipm_set_polish: steps = " + std::to_string(steps) + ", must be >= 0"; return TLPK_BADARG; }
    h->polish.ipm_steps = steps;
    return TLPK_OK;
}

/* HSD.jl:77-128 + the quantities of HSD.jl:136-196.  out[13]:
 *  0 |rp|inf  1 |rl|inf  2 |ru|inf  3 |rd|inf  4 c'x  5 b'y  6 lz'zl  7 uz'zu  8 xl'zl + xu'zu
 *  9 |A x|inf  10 |(x - xl) lflag|inf  11 |(x + xu) uflag|inf  12 |A'y + zl lflag - zu uflag|inf */
int tlpk_ipm_residuals(tlpk_handle *h, double tau, double *out) {
    Shards sh;
    if (int rc = ipm_shards(h, sh)) return rc;
    if (!out) return TLPK_BADARG;
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r]; IpmState &s = *c->ipm;
        HIPCHK(h, hipSetDevice(c->device));
        dense_products(c, true, true);
        const int nbc = ipm_launch_res_cols(c->stream, s.v, tau, s.partials[0]);
        const int nbr = ipm_launch_res_rows(c->stream, s.v, tau, s.partials[1]);
        ipm_launch_finalize(c->stream, nbc, 4, 6, 0, s.partials[0], s.d_out);
        ipm_launch_finalize(c->stream, nbr, 1, 2, 0, s.partials[1], s.d_out + IPM_SLOTS);
        if (sh.multi && h->ipm->h_link) {       // the shard's partial rp on the linking rows
            IpmState &ps = *h->ipm; const i64 len = ps.link_hi - ps.link_lo;
            HIPCHK(h, hipMemcpyAsync(ps.h_link + (size_t)r * (size_t)len, s.v.rp + ps.link_lo, (size_t)len * 8, hipMemcpyDeviceToHost, c->stream));
        }
    }
    double q[2 * IPM_SLOTS];
    if (int rc = gather2(h, sh, 4, 6, 10, 1, 2, 3, q)) return rc;
    const double *a = q, *r = q + IPM_SLOTS;
    double rp_inf = r[1], ax_inf = r[2];
    if (sh.multi && h->ipm->h_link) {
        // linking rows: rp = sum of the shards' partial rows (shard order), A x = tau b - rp
        IpmState &ps = *h->ipm; const i64 len = ps.link_hi - ps.link_lo;
        for (size_t k = 0; k < ps.link_rows.size(); ++k) {
            const i64 off = ps.link_rows[k] - ps.link_lo;
            double v = ps.h_link[off];
            for (int s2 = 1; s2 < sh.n; ++s2) v += ps.h_link[(size_t)s2 * (size_t)len + (size_t)off];
            rp_inf = std::fmax(rp_inf, std::fabs(v));
            ax_inf = std::fmax(ax_inf, std::fabs(tau * ps.b_link[k] - v));
        }
    }
    out[0] = rp_inf; out[1] = a[4]; out[2] = a[5]; out[3] = a[6]; out[4] = a[0]; out[5] = r[0]; out[6] = a[1]; out[7] = a[2];
    out[8] = a[3]; out[9] = ax_inf; out[10] = a[7]; out[11] = a[8]; out[12] = a[9];
    return TLPK_OK;
}

/* step.jl:24-51: theta_inv from the iterate, uniform regularisations, KKT.update!.  TLPK_NOT_POSDEF is
 * the PosDefException of the retry loop: call again with larger regularisations. */
int tlpk_ipm_factor(tlpk_handle *h, double regP, double regD) {
    Shards sh;
    if (int rc = ipm_shards(h, sh)) return rc;
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r];
        HIPCHK(h, hipSetDevice(c->device));
        ipm_launch_theta(c->stream, c->ipm->v, c->d_theta, c->d_regP, c->d_regD, regP, regD);
    }
    return update_all(h, sh);
}

/* step.jl:56-76: solve the h-system (xi_p = b, xi_d = c - th_l lz - th_u uz); hx, hy stay on the device.
 * out[0] = lz'(lz th_l) + uz'(uz th_u) - (c + th_l lz + th_u uz)'hx + b'hy   (the host adds kappa/tau + regG) */
int tlpk_ipm_hsolve(tlpk_handle *h, double *out) {
    Shards sh;
    if (int rc = ipm_shards(h, sh)) return rc;
    if (!out) return TLPK_BADARG;
    for (int r = 0; r < sh.n; ++r) { HIPCHK(h, hipSetDevice(sh.c[r]->device)); ipm_launch_hrhs(sh.c[r]->stream, sh.c[r]->ipm->v); }
    int rc = solve_all(h, sh, [](IpmState &s, double *&dx, double *&dy, const double *&xp, const double *&xd) { dx = s.v.hx; dy = s.v.hy; xp = s.v.b; xd = s.v.hxid; });
    if (rc != TLPK_OK) return rc;
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r]; IpmState &s = *c->ipm;
        HIPCHK(h, hipSetDevice(c->device));
        const int nb = ipm_launch_hdots(c->stream, s.v, s.partials[0]);
        ipm_launch_finalize(c->stream, nb, 2, 0, 0, s.partials[0], s.d_out);
    }
    double q[IPM_SLOTS];
    if ((rc = gather(h, sh, 2, 2, 0, q)) != TLPK_OK) return rc;
    if ((rc = sync_all(h, sh)) != TLPK_OK) return rc;
    out[0] = q[0] + q[1];
    return TLPK_OK;
}

/* step.jl:325-364 (first half of compute_higher_corrector): targets from the accepted direction;
 * out[0] = sum(vl), out[1] = sum(vu); the host adds the tau-kappa term and forms delta. */
int tlpk_ipm_targets(tlpk_handle *h, double a_, double mu_l, double mu_u, double *out) {
    Shards sh;
    if (int rc = ipm_shards(h, sh)) return rc;
    if (!out) return TLPK_BADARG;
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r]; IpmState &s = *c->ipm;
        HIPCHK(h, hipSetDevice(c->device));
        const int nb = ipm_launch_targets(c->stream, s.v, s.D[s.cur], a_, a_, mu_l, mu_u, s.partials[0]);
        ipm_launch_finalize(c->stream, nb, 2, 0, 0, s.partials[0], s.d_out);
    }
    double q[IPM_SLOTS];
    if (int rc = gather(h, sh, 2, 2, 0, q)) return rc;
    out[0] = q[0]; out[1] = q[1];
    return TLPK_OK;
}

/* step.jl:198-266 (solve_newton_system) + step.jl:294-306 (max step) for one right-hand side:
 *   mode 0 predictor, mode 1 corrector, mode 2 centrality corrector (after tlpk_ipm_targets).
 * sc[8] = { tau, kappa, h0, xi_g, xi_tk, eta, gamma*mu, delta }.
 * Modes 0 / 1 write the accepted direction, mode 2 writes the candidate (Dc = solution + accepted direction).
 * out[3] = { dtau, dkappa, largest step to the boundary over xl, xu, zl, zu (inf if none) } of the written
 * direction; for mode 2 dtau / dkappa are those of the solution alone (the host adds the accepted ones). */
int tlpk_ipm_newton(tlpk_handle *h, int mode, const double *sc, double *out) {
    Shards sh;
    if (int rc = ipm_shards(h, sh)) return rc;
    if (!sc || !out || mode < 0 || mode > 2) return TLPK_BADARG;
    const double tau = sc[0], kappa = sc[1], h0 = sc[2], xi_g = sc[3], xi_tk = sc[4], eta = sc[5], gmu = sc[6], delta = sc[7];
    int nb[MAX_DEVICES];
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r]; IpmState &s = *c->ipm;
        HIPCHK(h, hipSetDevice(c->device));
        nb[r] = ipm_launch_newton_pre(c->stream, s.v, s.D[s.cur], mode, eta, gmu, delta, s.partials[0]);
    }
    int rc = solve_all(h, sh, [mode](IpmState &s, double *&dx, double *&dy, const double *&xp, const double *&xd) {
        const IpmDir &dst = (mode == 2) ? s.D[1 - s.cur] : s.D[s.cur]; dx = dst.x; dy = dst.y; xp = s.v.xip; xd = s.v.xid; });
    if (rc != TLPK_OK) return rc;
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r]; IpmState &s = *c->ipm;
        const IpmDir &dst = (mode == 2) ? s.D[1 - s.cur] : s.D[s.cur];
        HIPCHK(h, hipSetDevice(c->device));
        ipm_launch_newton_dots(c->stream, s.v, dst, nb[r], s.partials[0]);
        ipm_launch_finalize(c->stream, nb[r], 6, 0, 0, s.partials[0], s.d_out);
    }
    double q[IPM_SLOTS];
    if ((rc = gather(h, sh, 6, 6, 0, q)) != TLPK_OK) return rc;
    if ((rc = sync_all(h, sh)) != TLPK_OK) return rc;
    // step.jl:232-246
    const double xi_g_ = xi_g + xi_tk / tau - q[0] + q[1] - q[2] - q[3];
    const double dtau = (xi_g_ + q[4] - q[5]) / h0;
    const double dkappa = (xi_tk - kappa * dtau) / tau;
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r]; IpmState &s = *c->ipm;
        const IpmDir &acc = s.D[s.cur];
        const IpmDir &dst = (mode == 2) ? s.D[1 - s.cur] : s.D[s.cur];
        HIPCHK(h, hipSetDevice(c->device));
        const int nb2 = ipm_launch_newton_post(c->stream, s.v, dst, acc, mode == 2 ? 1 : 0, dtau, s.partials[1]);
        ipm_launch_finalize(c->stream, nb2, 0, 0, 2, s.partials[1], s.d_out);
    }
    if ((rc = gather(h, sh, 2, 0, 0, q)) != TLPK_OK) return rc;
    out[0] = dtau; out[1] = dkappa; out[2] = std::fmin(q[0], q[1]);    // one step length for both sides
    return TLPK_OK;
}

/* step.jl:24-94 in ONE call: tlpk_ipm_factor (theta_inv from the iterate, uniform regularisations, KKT.update!) WITHOUT the wait for its
 * status, followed by tlpk_ipm_hsolve_newton: the block-level forward sweeps of the paired solve overlap the factorisation of the root
 * (linking) front (tlpk_update_device_async).  TLPK_NOT_POSDEF is returned where tlpk_ipm_factor would have returned it -- the
 * speculative solve has only written direction / h-system buffers -- and the caller retries with larger regularisations (step.jl:35-51).
 * Multi-device handles: the blocking factorisation, then tlpk_ipm_hsolve_newton. */
int tlpk_ipm_factor_hsolve_newton(tlpk_handle *h, double regP, double regD, const double *sc, double *out) {
    Shards sh;
    if (int rc = ipm_shards(h, sh)) return rc;
    if (!sc || !out) return TLPK_BADARG;
    if (sh.multi) { const int rc = tlpk_ipm_factor(h, regP, regD); return rc != TLPK_OK ? rc : tlpk_ipm_hsolve_newton(h, sc, out); }
    HIPCHK(h, hipSetDevice(h->device));
    ipm_launch_theta(h->stream, h->ipm->v, h->d_theta, h->d_regP, h->d_regD, regP, regD);
    const int rc = tlpk_update_device_async(h, h->d_theta, h->d_regP, h->d_regD);
    if (rc != TLPK_OK) return rc;
    return tlpk_ipm_hsolve_newton(h, sc, out);
}

/* step.jl:56-94 in ONE call: the h-system (step.jl:56-76) and the predictor's Newton system (mode 0 of tlpk_ipm_newton) are
 * independent right-hand sides against the same factor -- they share one pass over L (tlpk_solve2_device: the sweeps are bound by
 * the bytes of L; multi-device handles: the split-phase pair, two reductions of root right-hand sides).  sc[8] as for tlpk_ipm_newton, except sc[2] = regG (h0 = dot products +
 * kappa / tau + regG is formed here).  out[4] = { dtau, dkappa, largest step to the boundary, h0 }.  Same arithmetic as
 * tlpk_ipm_hsolve + tlpk_ipm_newton(mode 0): bit-identical vectors and scalars. */
int tlpk_ipm_hsolve_newton(tlpk_handle *h, const double *sc, double *out) {
    Shards sh;
    if (int rc = ipm_shards(h, sh)) return rc;
    if (!sc || !out) return TLPK_BADARG;
    const double tau = sc[0], kappa = sc[1], regG = sc[2], xi_g = sc[3], xi_tk = sc[4], eta = sc[5], gmu = sc[6], delta = sc[7];
    int nb[MAX_DEVICES];
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r]; IpmState &s = *c->ipm;
        HIPCHK(h, hipSetDevice(c->device));
        ipm_launch_hrhs(c->stream, s.v);
        nb[r] = ipm_launch_newton_pre(c->stream, s.v, s.D[s.cur], 0, eta, gmu, delta, s.partials[0]);
    }
    int rc;
    if (!sh.multi) {
        IpmState &s = *h->ipm; const IpmDir &dst = s.D[s.cur];
        rc = tlpk_solve2_device(h, s.v.hx, s.v.hy, s.v.b, s.v.hxid, dst.x, dst.y, s.v.xip, s.v.xid);
        if (rc == TLPK_OK && h->polish.ipm_steps > 0) rc = tlpk_polish2_device(h, s.v.hx, s.v.hy, s.v.b, s.v.hxid, dst.x, dst.y, s.v.xip, s.v.xid, h->polish.ipm_steps);
    } else {
        double *dx0[MAX_DEVICES], *dy0[MAX_DEVICES], *dx1[MAX_DEVICES], *dy1[MAX_DEVICES];
        const double *xp0[MAX_DEVICES], *xd0[MAX_DEVICES], *xp1[MAX_DEVICES], *xd1[MAX_DEVICES];
        for (int r = 0; r < sh.n; ++r) {
            IpmState &s = *sh.c[r]->ipm;
            dx0[r] = s.v.hx; dy0[r] = s.v.hy; xp0[r] = s.v.b; xd0[r] = s.v.hxid;
            dx1[r] = s.D[s.cur].x; dy1[r] = s.D[s.cur].y; xp1[r] = s.v.xip; xd1[r] = s.v.xid;
        }
        rc = multi_solve2_resident(h, dx0, dy0, xp0, xd0, dx1, dy1, xp1, xd1);
    }
    if (rc != TLPK_OK) return rc;
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r]; IpmState &s = *c->ipm; const IpmDir &dst = s.D[s.cur];
        HIPCHK(h, hipSetDevice(c->device));
        const int nbh = ipm_launch_hdots(c->stream, s.v, s.partials[1]);
        ipm_launch_finalize(c->stream, nbh, 2, 0, 0, s.partials[1], s.d_out + IPM_SLOTS);
        ipm_launch_newton_dots(c->stream, s.v, dst, nb[r], s.partials[0]);
        ipm_launch_finalize(c->stream, nb[r], 6, 0, 0, s.partials[0], s.d_out);
    }
    double q[2 * IPM_SLOTS];
    if ((rc = gather2(h, sh, 6, 0, 6, 2, 0, 2, q)) != TLPK_OK) return rc;
    if ((rc = sync_all(h, sh)) != TLPK_OK) return rc;
    const double h0 = ((q[IPM_SLOTS] + q[IPM_SLOTS + 1]) + kappa / tau) + regG;      // the association of hsd_device.py / HSD/step.jl:69-76
    const double xi_g_ = xi_g + xi_tk / tau - q[0] + q[1] - q[2] - q[3];
    const double dtau = (xi_g_ + q[4] - q[5]) / h0;
    const double dkappa = (xi_tk - kappa * dtau) / tau;
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r]; IpmState &s = *c->ipm; const IpmDir &dst = s.D[s.cur];
        HIPCHK(h, hipSetDevice(c->device));
        const int nb2 = ipm_launch_newton_post(c->stream, s.v, dst, dst, 0, dtau, s.partials[1]);
        ipm_launch_finalize(c->stream, nb2, 0, 0, 2, s.partials[1], s.d_out);
    }
    if ((rc = gather(h, sh, 2, 0, 0, q)) != TLPK_OK) return rc;
    out[0] = dtau; out[1] = dkappa; out[2] = std::fmin(q[0], q[1]); out[3] = h0;
    return TLPK_OK;
}

/* step.jl:112-118: the candidate of the last mode-2 call becomes the accepted direction */
int tlpk_ipm_accept(tlpk_handle *h) {
    Shards sh;
    if (int rc = ipm_shards(h, sh)) return rc;
    for (int r = 0; r < sh.n; ++r) sh.c[r]->ipm->cur = 1 - sh.c[r]->ipm->cur;
    return TLPK_OK;
}

/* step.jl:139-148: pt += alpha * D; out[0] = xl'zl + xu'zu of the new point (mu numerator, point.jl:45-48) */
static int advance_all(tlpk_handle *h, double ap, double ad, double *out) {
    Shards sh;
    if (int rc = ipm_shards(h, sh)) return rc;
    if (!out) return TLPK_BADARG;
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r]; IpmState &s = *c->ipm;
        HIPCHK(h, hipSetDevice(c->device));
        const int nb = ipm_launch_advance(c->stream, s.v, s.D[s.cur], ap, ad, s.partials[0]);
        ipm_launch_finalize(c->stream, nb, 1, 0, 0, s.partials[0], s.d_out);
    }
    double q[IPM_SLOTS];
    if (int rc = gather(h, sh, 1, 1, 0, q)) return rc;
    out[0] = q[0];
    return TLPK_OK;
}
int tlpk_ipm_advance(tlpk_handle *h, double alpha, double *out) { return advance_all(h, alpha, alpha, out); }

// the device vector behind every code of tlpk_ipm_get on handle c, and whether a code names a vector of length m
static void ipm_get_sources(const tlpk_handle *c, const double *src[36]) {
    const IpmState &s = *c->ipm; const IpmVecs &v = s.v;
    const IpmDir &acc = s.D[s.cur], &cand = s.D[1 - s.cur];
    const double *all[36] = {v.x, v.xl, v.xu, v.zl, v.zu, v.y,
                             acc.x, acc.xl, acc.xu, acc.zl, acc.zu, acc.y, cand.x, cand.xl, cand.xu, cand.zl, cand.zu, cand.y,
                             v.rp, v.rl, v.ru, v.rd, v.thl, v.thu, v.hx, v.hy, v.hxid, v.xil, v.xiu, v.xzl, v.xzu, v.xid, v.xip,
                             c->d_theta, c->d_regP, c->d_regD};
    std::copy(all, all + 36, src);
}
static bool ipm_get_is_row(int what) { return what == 5 || what == 11 || what == 17 || what == 18 || what == 25 || what == 32 || what == 35; }

/* download one device vector, read-only (nothing here writes device state):
 *   0-5    the iterate x, xl, xu, zl, zu (n), y (m)
 *   6-11   the accepted direction, same order (D[cur]);  12-17  the candidate direction (D[1 - cur])
 *   18-21  rp (m), rl, ru, rd          22-26  thl, thu, hx, hy (m), hxid          27-32  xil, xiu, xzl, xzu, xid, xip (m)
 *   33-35  the handle's theta_inv (n), regP (n), regD (m) as the last factor call wrote them
 * Codes above 5 serve single-device handles (batch-loaded ones included: stacked vectors); tests read the kernels' work through them. */
int tlpk_ipm_get(tlpk_handle *h, int what, double *host, int64_t len) {
    Shards sh;
    if (int rc = ipm_shards(h, sh, true, true, true)) return rc;
    if (!host || what < 0 || what > 35) return TLPK_BADARG;
    if (sh.multi && what > 5) { h->last_error = "tlpk_ipm_get: the codes 6 .. 35 (directions, residuals, right-hand sides, theta) need a single-device handle"; return TLPK_BADARG; }
    const IpmVecs &v0 = sh.c[0]->ipm->v;
    const int64_t need = ipm_get_is_row(what) ? v0.m : v0.n;
    if (len != need) { h->last_error = "tlpk_ipm_get: wrong length"; return TLPK_BADARG; }
    std::vector<double> tmp;
    if (sh.multi) tmp.resize((size_t)std::max<int64_t>(need, 1));
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r];
        const double *src[36];
        ipm_get_sources(c, src);
        HIPCHK(h, hipSetDevice(c->device));
        HIPCHK(h, hipStreamSynchronize(c->stream));
        if (need <= 0) continue;
        if (!src[what]) { h->last_error = "tlpk_ipm_get: the handle does not hold that vector"; return TLPK_BADARG; }
        if (!sh.multi) { HIPCHK(h, hipMemcpy(host, src[what], (size_t)need * 8, hipMemcpyDeviceToHost)); continue; }
        // every entry from the shard that owns it (linking rows: the lead)
        HIPCHK(h, hipMemcpy(tmp.data(), src[what], (size_t)need * 8, hipMemcpyDeviceToHost));
        const bool k2 = c->S.system == 1;
        const std::vector<char> &rl = c->S.row_local;
        if (what == 5) { const int64_t off = k2 ? c->S.k2_n : 0; for (int64_t i = 0; i < need; ++i) { const char q = rl[(size_t)(off + i)]; if (q == 1 || (q == 2 && r == 0)) host[i] = tmp[(size_t)i]; } }
        else if (k2) { for (int64_t j = 0; j < need; ++j) { const char q = rl[(size_t)j]; if (q == 1 || (q == 2 && r == 0)) host[j] = tmp[(size_t)j]; } }
        else { const std::vector<char> &cl = c->S.col_local; for (int64_t j = 0; j < need; ++j) if (cl[(size_t)j]) host[j] = tmp[(size_t)j]; }
    }
    return TLPK_OK;
}

/* ---- Mehrotra predictor-corrector with the iterate in HBM (MPC/MPC.jl, MPC/step.jl) ------------------------
 * Shares the vectors, tlpk_ipm_load / residuals (tau = 1) / factor / accept / get with the HSD entry points. */

/* MPC.jl:353-410: starting point.  One factorisation of A A' + 1e-6 I, two solves with a zero half of the
 * right-hand side, shifts to positive coordinates, balanced products.  out[0] = xl'zl + xu'zu. */
int tlpk_mpc_start(tlpk_handle *h, double *out) {
    Shards sh;
    if (int rc = ipm_shards(h, sh)) return rc;
    if (!out) return TLPK_BADARG;
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r];
        HIPCHK(h, hipSetDevice(c->device));
        mpc_launch_fill(c->stream, c->ipm->v, c->d_theta, c->d_regP, c->d_regD);
    }
    int rc = update_all(h, sh);
    if (rc != TLPK_OK) return rc;
    rc = solve_all(h, sh, [](IpmState &s, double *&dx, double *&dy, const double *&xp, const double *&xd) { dx = s.D[0].x; dy = s.v.y; xp = s.v.xip; xd = s.v.c; });      // y  (xip == 0 here)
    if (rc != TLPK_OK) return rc;
    rc = solve_all(h, sh, [](IpmState &s, double *&dx, double *&dy, const double *&xp, const double *&xd) { dx = s.v.x; dy = s.D[0].y; xp = s.v.b; xd = s.v.xid; });      // x  (xid == 0 here)
    if (rc != TLPK_OK) return rc;
    double q[IPM_SLOTS];
    auto stage = [&](int st, double a, double b, int nsum, int nmin) -> int {
        for (int r = 0; r < sh.n; ++r) {
            tlpk_handle *c = sh.c[r]; IpmState &s = *c->ipm;
            HIPCHK(h, hipSetDevice(c->device));
            if (st == 2) dense_products(c, true, false);
            const int nb = mpc_launch_start(c->stream, s.v, st, a, b, s.partials[0]);
            ipm_launch_finalize(c->stream, nb, nsum, 0, nmin, s.partials[0], s.d_out);
        }
        return gather(h, sh, nsum + nmin, nsum, 0, q);
    };
    if ((rc = stage(1, 0.0, 0.0, 0, 2)) != TLPK_OK) return rc;
    if ((rc = sync_all(h, sh)) != TLPK_OK) return rc;
    const double dxs = 1.0 + std::fmax(0.0, std::fmax(-1.5 * q[0], -1.5 * q[1]));
    if ((rc = stage(2, dxs, 0.0, 0, 2)) != TLPK_OK) return rc;
    const double dzs = 1.0 + std::fmax(0.0, std::fmax(-1.5 * q[0], -1.5 * q[1]));
    if ((rc = stage(3, dzs, 0.0, 3, 0)) != TLPK_OK) return rc;
    const double mu = q[0], ddx = mu / (2.0 * q[1]), ddz = mu / (2.0 * q[2]);
    if ((rc = stage(4, ddx, ddz, 1, 0)) != TLPK_OK) return rc;
    out[0] = q[0];
    for (int r = 0; r < sh.n; ++r) sh.c[r]->ipm->cur = 0;
    return TLPK_OK;
}

/* MPC/step.jl:164-217 (solve_newton_system + max_step_length_pd) for one right-hand side:
 *   mode 0 predictor (xi = residuals, complementarity -x z), mode 1 corrector (same residuals, sigma mu - x z - dx dz
 *   with the predictor direction, which it overwrites; gmu = sigma mu), mode 2 centrality corrector (zero residuals,
 *   the targets of tlpk_mpc_targets; writes the candidate = solution + accepted direction).
 * out[2] = largest primal step (over xl, xu) and largest dual step (over zl, zu) to the boundary, inf if none. */
int tlpk_mpc_newton(tlpk_handle *h, int mode, double gmu, double *out) {
    Shards sh;
    if (int rc = ipm_shards(h, sh)) return rc;
    if (!out || mode < 0 || mode > 2) return TLPK_BADARG;
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r]; IpmState &s = *c->ipm;
        HIPCHK(h, hipSetDevice(c->device));
        ipm_launch_newton_pre(c->stream, s.v, s.D[s.cur], mode, 1.0, gmu, 0.0, s.partials[0]);
    }
    int rc = solve_all(h, sh, [mode](IpmState &s, double *&dx, double *&dy, const double *&xp, const double *&xd) {
        const IpmDir &dst = (mode == 2) ? s.D[1 - s.cur] : s.D[s.cur]; dx = dst.x; dy = dst.y; xp = s.v.xip; xd = s.v.xid; });
    if (rc != TLPK_OK) return rc;
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r]; IpmState &s = *c->ipm;
        const IpmDir &acc = s.D[s.cur];
        const IpmDir &dst = (mode == 2) ? s.D[1 - s.cur] : s.D[s.cur];
        HIPCHK(h, hipSetDevice(c->device));
        const int nb = ipm_launch_newton_post(c->stream, s.v, dst, acc, mode == 2 ? 1 : 0, 0.0, s.partials[1]);   // dtau = 0: hx, hy (zeros) unused
        ipm_launch_finalize(c->stream, nb, 0, 0, 2, s.partials[1], s.d_out);
    }
    double q[IPM_SLOTS];
    if ((rc = gather(h, sh, 2, 0, 0, q)) != TLPK_OK) return rc;
    if ((rc = sync_all(h, sh)) != TLPK_OK) return rc;
    out[0] = q[0]; out[1] = q[1];
    return TLPK_OK;
}

/* MPC/step.jl:246-258, 290-296: out[0] = complementarity of the point moved by (ap, ad) along the accepted direction,
 * out[1] = xl'zl + xu'zu of the point itself */
int tlpk_mpc_gap(tlpk_handle *h, double ap, double ad, double *out) {
    Shards sh;
    if (int rc = ipm_shards(h, sh)) return rc;
    if (!out) return TLPK_BADARG;
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r]; IpmState &s = *c->ipm;
        HIPCHK(h, hipSetDevice(c->device));
        const int nb = mpc_launch_gap(c->stream, s.v, s.D[s.cur], ap, ad, s.partials[0]);
        ipm_launch_finalize(c->stream, nb, 2, 0, 0, s.partials[0], s.d_out);
    }
    double q[IPM_SLOTS];
    if (int rc = gather(h, sh, 2, 2, 0, q)) return rc;
    out[0] = q[0]; out[1] = q[1];
    return TLPK_OK;
}

/* MPC/step.jl:329-358 (compute_target!): targets of the centrality corrector from the accepted direction at the trial
 * step lengths (ap_, ad_), box [tmin, tmax]; they stay on the device for tlpk_mpc_newton(mode 2) */
int tlpk_mpc_targets(tlpk_handle *h, double ap_, double ad_, double tmin, double tmax) {
    Shards sh;
    if (int rc = ipm_shards(h, sh)) return rc;
    for (int r = 0; r < sh.n; ++r) {
        tlpk_handle *c = sh.c[r]; IpmState &s = *c->ipm;
        HIPCHK(h, hipSetDevice(c->device));
        ipm_launch_targets(c->stream, s.v, s.D[s.cur], ap_, ad_, tmin, tmax, s.partials[0]);
    }
    return TLPK_OK;
}

/* MPC/step.jl:112-123: primal side += ap * D, dual side += ad * D; out[0] = xl'zl + xu'zu of the new point */
int tlpk_mpc_advance(tlpk_handle *h, double ap, double ad, double *out) { return advance_all(h, ap, ad, out); }

/* ---- a stack of LPs on one handle (include/tlpk.h, "Batched device-resident HSD"; DESIGN.md section 4b') -------------------------------
 * B LPs stacked into one block-diagonal A are an ordinary handle: the level-batched factorisation and solve kernels serve every block in
 * the launches one block needs.  What these calls add is the interior-point loop with PER-LP scalars: the kernels of
 * ipm_batch_kernels.hip, the scalar algebra between them once per LP, and `active` masks (an LP whose flag is 0 is not touched). */
}  // extern "C"

namespace {

// the stacked-LP state of a handle, or the reason why there is none
int batch_state(tlpk_handle *h, IpmBatchState *&bs) {
    if (!h) return TLPK_BADARG;
    if (!h->ipm) { h->last_error = "tlpk_ipm_load_batch has not been called (load first)"; return TLPK_BADARG; }
    if (!h->ipm->bat) { h->last_error = "the handle holds one LP (tlpk_ipm_load): the tlpk_ipm_batch_* calls need tlpk_ipm_load_batch"; return TLPK_BADARG; }
    if (!h->has_device) return TLPK_NO_DEVICE;
    if (h->ipm_stale) {
        h->last_error = "the matrix values changed (tlpk_set_values) after the LPs were loaded: call tlpk_ipm_reload before the device-resident loops";
        return TLPK_BADARG;
    }
    bs = h->ipm->bat;
    return TLPK_OK;
}
// the scalars of this call: sc(k, q) for q < IPM_BSC - 1, the flags (nullptr: every LP).  The previous call (or half of a call) has been waited for.
template <class F>
int batch_scalars(tlpk_handle *h, IpmBatchState &bs, const uint8_t *active, F &&sc) {
    for (i64 k = 0; k < bs.nlp; ++k) {
        double *row = bs.h_sc + (size_t)k * IPM_BSC;
        for (int q = 0; q < IPM_BSC - 1; ++q) row[q] = sc(k, q);
        row[IPM_BSC - 1] = (!active || active[k]) ? 1.0 : 0.0;
    }
    HIPCHK(h, hipMemcpyAsync(bs.d_sc, bs.h_sc, (size_t)bs.nlp * IPM_BSC * 8, hipMemcpyHostToDevice, h->stream));
    return TLPK_OK;
}
// the finalised scalars of `groups` reductions (group g at d_out + g nlp IPM_SLOTS): copy, wait
int batch_gather(tlpk_handle *h, IpmBatchState &bs, int groups) {
    HIPCHK(h, hipMemcpyAsync(bs.h_out, bs.d_out, (size_t)groups * (size_t)bs.nlp * IPM_SLOTS * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    return TLPK_OK;
}
// which LP owns node `col` of the factored matrix (tlpk_stats.fail_col: a permuted index), or -1
i64 batch_owner(const tlpk_handle *h, const IpmBatchState &bs, i64 col) {
    const Symbolic &S = h->S;
    if (col < 0 || col >= (i64)S.perm.size()) return -1;
    i64 old = S.perm[(size_t)col];
    const std::vector<i64> *off = &bs.row_off;
    if (S.system == 1) { if (old < S.k2_n) off = &bs.col_off; else old -= S.k2_n; }      // K2: node j < n is a column, n + i a row
    if (old < 0 || old >= off->back()) return -1;
    return (i64)(std::upper_bound(off->begin(), off->end(), old) - off->begin()) - 1;
}
// the fronts of every LP, verified (skip_build_units): what tlpk_ipm_batch_skip and a hold of tlpk_ipm_batch_factor_each need before a block can be left out
int batch_unit_tables(tlpk_handle *h, const IpmBatchState &bs, const char *what, bool allow_shared = false) {
    if (!h->front_unit.empty() && h->skip_units_batch && (allow_shared || !h->units_shared)) return TLPK_OK;
    // (a table that tlpk_block_skip built before the load names the blocks of row_block, which need not be the LPs: rebuilt, and its device copy refreshed)
    std::vector<i32> ru((size_t)bs.row_off.back()), cu((size_t)bs.col_off.back());
    for (i64 k = 0; k < bs.nlp; ++k) {
        std::fill(ru.begin() + bs.row_off[(size_t)k], ru.begin() + bs.row_off[(size_t)k + 1], (i32)k);
        std::fill(cu.begin() + bs.col_off[(size_t)k], cu.begin() + bs.col_off[(size_t)k + 1], (i32)k);
    }
    if (int rc = skip_build_units(h, ru, cu, bs.nlp, what, allow_shared)) return rc;
    h->skip_units_batch = true;
    if (h->d.front_unit) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(h->d.front_unit, h->front_unit.data(), h->front_unit.size() * sizeof(i32), hipMemcpyHostToDevice));
    }
    return TLPK_OK;
}
// tlpk_ipm_batch_skip: the update / the solves enqueued while a MaskScope lives leave out the LPs whose flag in the call's scalar block is 0 -- the copy
// batch_scalars has just enqueued, expanded per front on the same stream; no mask is in force once the scope ends
struct MaskScope {
    tlpk_handle *h; int rc = TLPK_OK;
    MaskScope(tlpk_handle *h_, IpmBatchState &bs, int slot = IPM_BSC - 1) : h(h_) { if (h->batch_skip) rc = skip_from_flags(h, bs.d_sc + slot, IPM_BSC); }
    ~MaskScope() { skip_off(h); }
};
// step.jl:232-246 for one LP, from the six sums of the pre / dots kernels
inline void newton_scalars(const double *q, double tau, double kappa, double h0, double xi_g, double xi_tk, double &dtau, double &dkappa) {
    const double xi_g_ = xi_g + xi_tk / tau - q[0] + q[1] - q[2] - q[3];
    dtau = (xi_g_ + q[4] - q[5]) / h0;
    dkappa = (xi_tk - kappa * dtau) / tau;
}

}  // namespace

extern "C" {

int tlpk_ipm_load_batch(tlpk_handle *h, int64_t nlp, const int64_t *row_off, const int64_t *col_off,
                        const double *b, const double *c, const double *l, const double *u) {
    if (!h) return TLPK_BADARG;
    // 1. the arguments themselves
    if (!row_off || !col_off || !b || !c || !l || !u) { h->last_error = "tlpk_ipm_load_batch: a NULL pointer"; return TLPK_BADARG; }
    if (nlp < 1) { h->last_error = "tlpk_ipm_load_batch: nlp must be at least 1"; return TLPK_BADARG; }
    // 2. the offsets
    const Symbolic &S = h->S;
    const bool k2 = S.system == 1;
    const i64 m = k2 ? S.k2_m : S.m - S.n_dense, n = k2 ? S.k2_n : S.n;
    if (row_off[0] != 0 || col_off[0] != 0) { h->last_error = "tlpk_ipm_load_batch: the offsets must start at 0"; return TLPK_BADARG; }
    for (i64 k = 0; k < nlp; ++k) {
        if (row_off[k + 1] < row_off[k] || col_off[k + 1] < col_off[k]) { h->last_error = "tlpk_ipm_load_batch: the offsets must not decrease (LP " + std::to_string(k) + ")"; return TLPK_BADARG; }
        if (row_off[k + 1] == row_off[k] || col_off[k + 1] == col_off[k]) { h->last_error = "tlpk_ipm_load_batch: LP " + std::to_string(k) + " is an empty segment (no rows or no columns)"; return TLPK_BADARG; }
    }
    if (row_off[nlp] != m || col_off[nlp] != n) {
        h->last_error = "tlpk_ipm_load_batch: the offsets must end at m = " + std::to_string(m) + " and n = " + std::to_string(n);
        return TLPK_BADARG;
    }
    // 3. every stored entry of A inside its LP's diagonal block: one walk of the handle's column-major copy (K2: the incidence matrix of
    //    the augmented system -- column p holds entry p of A as the pair variable node j, constraint node n + i)
    const bool has_csc = !S.dense_matrix && S.Ap.size() == (size_t)S.n + 1;
    if (has_csc && !k2) {
        i64 k = 0;
        for (i64 j = 0; j < n; ++j) {
            while (j >= col_off[k + 1]) ++k;
            for (i64 q = S.Ap[(size_t)j]; q < S.Ap[(size_t)j + 1]; ++q) {
                const i64 i = S.Ai[(size_t)q];
                if (i >= m) continue;                                     // (not a constraint row of the caller's matrix)
                if (i < row_off[k] || i >= row_off[k + 1]) {
                    h->last_error = "tlpk_ipm_load_batch: entry (" + std::to_string(i) + ", " + std::to_string(j) + ") of A lies outside the diagonal block of LP " + std::to_string(k);
                    return TLPK_BADARG;
                }
            }
        }
    } else if (has_csc) {
        for (i64 p = 0; p < S.n; ++p) {
            if (S.Ap[(size_t)p + 1] - S.Ap[(size_t)p] != 2) { h->last_error = "K2 incidence matrix: unexpected column"; return TLPK_INTERNAL; }
            const i64 q = S.Ap[(size_t)p];
            const i64 a = S.Ai[(size_t)q], b2 = S.Ai[(size_t)q + 1];
            const i64 j = std::min(a, b2), i = std::max(a, b2) - n;
            if (j < 0 || j >= n || i < 0 || i >= m) { h->last_error = "K2 incidence matrix: unexpected column"; return TLPK_INTERNAL; }
            const i64 k = (i64)(std::upper_bound(col_off, col_off + nlp + 1, j) - col_off) - 1;
            if (i < row_off[k] || i >= row_off[k + 1]) {
                h->last_error = "tlpk_ipm_load_batch: entry (" + std::to_string(i) + ", " + std::to_string(j) + ") of A lies outside the diagonal block of LP " + std::to_string(k);
                return TLPK_BADARG;
            }
        }
    }
    // the kind of handle
    const char *why = nullptr;
    if (!h->sub.empty()) why = "a multi-device handle";
    else if (h->opt.nranks > 1) why = "a sharded handle";
    else if (S.dense_matrix) why = "a dense-matrix handle";
    else if (h->krylov) why = "a matrix-free (Krylov) handle";
    else if (S.n_dense > 0) why = "a handle with dense columns (dense_cols)";
    if (why) { h->last_error = std::string("tlpk_ipm_load_batch: ") + why + " cannot hold a stack of LPs (single-device direct handles, K1 or K2, only)"; return TLPK_BADARG; }
    if (h->ipm) { h->last_error = "tlpk_ipm_load_batch: an LP is already loaded on this handle (tlpk_ipm_load or tlpk_ipm_load_batch)"; return TLPK_BADARG; }
    if (!h->has_device) return TLPK_NO_DEVICE;

    int rc = ipm_load_impl(h, b, c, l, u, false);
    IpmBatchState *bs = nullptr;
    if (rc == TLPK_OK) { bs = new (std::nothrow) IpmBatchState(); if (!bs) rc = TLPK_OOM; }
    if (rc == TLPK_OK) {
        h->ipm->bat = bs;
        rc = [&]() -> int {
            bs->nlp = nlp;
            bs->row_off.assign(row_off, row_off + nlp + 1); bs->col_off.assign(col_off, col_off + nlp + 1);
            IpmBatch &B = bs->B;
            B.nlp = nlp;
            i64 *dp;
            if (int r = dev_upload(h, &dp, bs->row_off)) return r; B.row_off = dp;
            if (int r = dev_upload(h, &dp, bs->col_off)) return r; B.col_off = dp;
            // block tables: LP k gets the blocks the unbatched kernels launch for its lengths
            auto table = [&](IpmBlockTab &t, auto len) -> int {
                std::vector<int> seg, loc, first((size_t)nlp + 1, 0);
                for (i64 k = 0; k < nlp; ++k) {
                    const int nb = ipm_seg_blocks(len(k));
                    if ((i64)seg.size() + nb > (i64)1 << 30) { h->last_error = "tlpk_ipm_load_batch: too many workgroups"; return TLPK_TOO_LARGE; }
                    for (int q = 0; q < nb; ++q) { seg.push_back((int)k); loc.push_back(q); }
                    first[(size_t)k + 1] = (int)seg.size();
                }
                int *di;
                t.nblocks = (int)seg.size();
                if (int r = dev_upload(h, &di, seg)) return r; t.seg = di;
                if (int r = dev_upload(h, &di, loc)) return r; t.loc = di;
                if (int r = dev_upload(h, &di, first)) return r; t.first = di;
                return TLPK_OK;
            };
            if (int r = table(B.tc, [&](i64 k) { return col_off[k + 1] - col_off[k]; })) return r;
            if (int r = table(B.tr, [&](i64 k) { return row_off[k + 1] - row_off[k]; })) return r;
            if (int r = table(B.tb, [&](i64 k) { return std::max(col_off[k + 1] - col_off[k], row_off[k + 1] - row_off[k]); })) return r;
            const i64 rows = std::max(B.tb.nblocks, std::max(B.tc.nblocks, B.tr.nblocks));
            double *p;
            for (int g = 0; g < 2; ++g) {
                if (int r = dev_alloc(h, &p, rows * IPM_SLOTS)) return r;
                HIPCHK(h, hipMemset(p, 0, (size_t)rows * IPM_SLOTS * 8));
                bs->partials[g] = p;
            }
            if (int r = dev_alloc(h, &p, 2 * nlp * IPM_SLOTS)) return r;
            HIPCHK(h, hipMemset(p, 0, (size_t)(2 * nlp * IPM_SLOTS) * 8)); bs->d_out = p;
            // (one row more than LPs, all ones and never overwritten: the flags of the unit that fronts shared by several LPs belong to -- batch_unit_tables)
            if (int r = dev_alloc(h, &p, (nlp + 1) * IPM_BSC)) return r;
            HIPCHK(h, hipMemset(p, 0, (size_t)(nlp * IPM_BSC) * 8)); bs->d_sc = p; B.sc = p;
            { const std::vector<double> ones((size_t)IPM_BSC, 1.0); HIPCHK(h, hipMemcpy(p + nlp * IPM_BSC, ones.data(), IPM_BSC * 8, hipMemcpyHostToDevice)); }
            for (int g = 0; g < 2; ++g) {
                if (int r = dev_alloc(h, &p, n)) return r;
                HIPCHK(h, hipMemset(p, 0, (size_t)std::max<i64>(n, 1) * 8)); bs->sx[g] = p;
                if (int r = dev_alloc(h, &p, m)) return r;
                HIPCHK(h, hipMemset(p, 0, (size_t)std::max<i64>(m, 1) * 8)); bs->sy[g] = p;
            }
            HIPCHK(h, hipHostMalloc((void **)&bs->h_out, (size_t)(2 * nlp * IPM_SLOTS) * 8, hipHostMallocDefault));
            HIPCHK(h, hipHostMalloc((void **)&bs->h_sc, (size_t)(nlp * IPM_BSC) * 8, hipHostMallocDefault));
            return TLPK_OK;
        }();
    }
    if (rc != TLPK_OK) ipm_free(h);
    else { skip_off(h); h->skip_host.clear(); }      // the batch owns the mask from here on: one that tlpk_block_skip set before the load is lifted
    return rc;
}

/* tlpk_ipm_residuals per LP: out[13 k ..] in its layout, from tau[k] */
int tlpk_ipm_batch_residuals(tlpk_handle *h, const double *tau, double *out) {
    IpmBatchState *bp = nullptr;
    if (int rc = batch_state(h, bp)) return rc;
    if (!tau || !out) return TLPK_BADARG;
    IpmBatchState &bs = *bp; IpmState &s = *h->ipm; const i64 nlp = bs.nlp;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = batch_scalars(h, bs, nullptr, [&](i64 k, int q) { return q == 0 ? tau[k] : 0.0; })) return rc;
    ipmb_launch_res_cols(h->stream, s.v, bs.B, bs.partials[0]);
    ipmb_launch_res_rows(h->stream, s.v, bs.B, bs.partials[1]);
    ipmb_launch_finalize(h->stream, bs.B, bs.B.tc, 4, 6, 0, bs.partials[0], bs.d_out);
    ipmb_launch_finalize(h->stream, bs.B, bs.B.tr, 1, 2, 0, bs.partials[1], bs.d_out + nlp * IPM_SLOTS);
    if (int rc = batch_gather(h, bs, 2)) return rc;
    for (i64 k = 0; k < nlp; ++k) {
        const double *a = bs.h_out + (size_t)k * IPM_SLOTS, *r = bs.h_out + (size_t)(nlp + k) * IPM_SLOTS;
        double *o = out + 13 * k;
        o[0] = r[1]; o[1] = a[4]; o[2] = a[5]; o[3] = a[6]; o[4] = a[0]; o[5] = r[0]; o[6] = a[1]; o[7] = a[2];
        o[8] = a[3]; o[9] = r[2]; o[10] = a[7]; o[11] = a[8]; o[12] = a[9];
    }
    return TLPK_OK;
}

/* tlpk_ipm_factor with regP[k] / regD[k] uniform within LP k; an LP with active[k] = 0 is parked (theta_inv = Rp = Rd = 1 on its block).
 * TLPK_NOT_POSDEF: *fail_lp = the LP that owns tlpk_stats.fail_col (-1 if it cannot be told); otherwise *fail_lp = -1. */
int tlpk_ipm_batch_factor(tlpk_handle *h, const uint8_t *active, const double *regP, const double *regD, int64_t *fail_lp) {
    IpmBatchState *bp = nullptr;
    if (int rc = batch_state(h, bp)) return rc;
    if (!active || !regP || !regD || !fail_lp) return TLPK_BADARG;
    IpmBatchState &bs = *bp;
    *fail_lp = -1;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = batch_scalars(h, bs, active, [&](i64 k, int q) { return q == 0 ? regP[k] : (q == 1 ? regD[k] : 0.0); })) return rc;
    ipmb_launch_theta(h->stream, h->ipm->v, bs.B, h->d_theta, h->d_regP, h->d_regD);
    MaskScope mask(h, bs);
    if (mask.rc != TLPK_OK) return mask.rc;
    const int rc = tlpk_update_device(h, h->d_theta, h->d_regP, h->d_regD);
    if (rc == TLPK_NOT_POSDEF) *fail_lp = batch_owner(h, bs, h->fail_col);
    return rc;
}

/* One update with a role per LP and a verdict per LP (include/tlpk.h; DESIGN.md section 4b'-v).  The pivot kernels mark every column they report
 * (the words behind DevCtx.info's status words); only an update whose status word says "failed" pays the fold of the marks and the copy of the nlp verdicts. */
int tlpk_ipm_batch_factor_each(tlpk_handle *h, const uint8_t *role, const double *regP, const double *regD, int64_t *fail_col, int64_t *nfail) {
    const char *me = "tlpk_ipm_batch_factor_each";
    if (!h) return TLPK_BADARG;
    if (!h->ipm) { h->last_error = "tlpk_ipm_load_batch has not been called (load first)"; return TLPK_BADARG; }
    if (!h->ipm->bat) { h->last_error = "the handle holds one LP (tlpk_ipm_load): the tlpk_ipm_batch_* calls need tlpk_ipm_load_batch"; return TLPK_BADARG; }
    if (!role || !regP || !regD || !fail_col || !nfail) { h->last_error = std::string(me) + ": a NULL pointer"; return TLPK_BADARG; }
    IpmBatchState &bs = *h->ipm->bat;
    const i64 nlp = bs.nlp;
    bool hold = false;
    for (i64 k = 0; k < nlp; ++k) {
        if (role[k] > 3) {
            h->last_error = std::string(me) + ": LP " + std::to_string(k) + " has role " + std::to_string((int)role[k]) + " (0 parked, 1 active, 2 hold, 3 entering)";
            return TLPK_BADARG;
        }
        hold = hold || role[k] == 2;
    }
    if (h->ipm_stale) {
        h->last_error = "the matrix values changed (tlpk_set_values) after the LPs were loaded: call tlpk_ipm_reload before the device-resident loops";
        return TLPK_BADARG;
    }
    if (hold) {      // a held block is left out of the update: the conditions of tlpk_ipm_batch_skip
        // (both sentences start with "...: hold refused": what the loops of batch_retry.py tell from every other TLPK_BADARG)
        if (h->refine_steps > 0) { h->last_error = std::string(me) + ": hold refused: refine_steps > 0: the norms of the refinement run over all rows"; return TLPK_BADARG; }
        // (a front that LPs share and that stands alone is tolerated: it is factorised by every call, from values that a held LP's segments still hold)
        if (int rc = batch_unit_tables(h, bs, "tlpk_ipm_batch_factor_each: hold refused", true)) return rc;
    }
    if (!h->has_device) return TLPK_NO_DEVICE;
    for (i64 k = 0; k < nlp; ++k) fail_col[k] = -1;
    *nfail = 0;
    HIPCHK(h, hipSetDevice(h->device));
    DevArrays &d = h->d;
    if (!d.unit_fail) {
        std::vector<i32> cu((size_t)h->S.m);
        for (i64 j = 0; j < h->S.m; ++j) cu[(size_t)j] = (i32)batch_owner(h, bs, j);
        i32 *dcu = nullptr; int *uf = nullptr;
        if (int rc = dev_upload(h, &dcu, cu)) return rc;
        if (int rc = dev_alloc(h, &uf, nlp)) return rc;
        if (!bs.h_fail) HIPCHK(h, hipHostMalloc((void **)&bs.h_fail, (size_t)nlp * sizeof(int), hipHostMallocDefault));
        d.col_unit = dcu; d.unit_fail = uf;
    }
    // the scalars: regP, regD (read for the active LPs only), the flag the mask is expanded from (1 = this update factorises the block), the role
    const bool masked = hold || h->batch_skip;
    for (i64 k = 0; k < nlp; ++k) {
        double *row = bs.h_sc + (size_t)k * IPM_BSC;
        const int r = role[k];
        for (int q = 0; q < IPM_BSC; ++q) row[q] = 0.0;
        if (r == 1) { row[0] = regP[k]; row[1] = regD[k]; }
        row[2] = (r == 1 || r == 3 || (r == 0 && !h->batch_skip)) ? 1.0 : 0.0;
        row[IPM_ROLE] = r == 1 ? IPM_ACTIVE : (r == 2 ? IPM_HOLD : (r == 3 ? IPM_ENTERING : IPM_PARKED));
        row[IPM_BSC - 1] = r == 1 ? 1.0 : 0.0;
    }
    HIPCHK(h, hipMemcpyAsync(bs.d_sc, bs.h_sc, (size_t)nlp * IPM_BSC * 8, hipMemcpyHostToDevice, h->stream));
    ipmb_launch_theta_roles(h->stream, h->ipm->v, bs.B, h->d_theta, h->d_regP, h->d_regD);
    if (masked) if (int rc = skip_from_flags(h, bs.d_sc + 2, IPM_BSC)) return rc;
    if (h->S.m > 0) HIPCHK(h, hipMemsetAsync(d.ctx.info + INFO_WORDS, 0x7f, (size_t)h->S.m * sizeof(int), h->stream));      // FAIL_NONE: no column is marked
    const int rc = tlpk_update_device(h, h->d_theta, h->d_regP, h->d_regD);
    skip_off(h);
    if (rc != TLPK_NOT_POSDEF) return rc;
    HIPCHK(h, hipMemsetAsync(d.unit_fail, 0x7f, (size_t)nlp * sizeof(int), h->stream));
    launch_fold_fail(h->stream, d);
    HIPCHK(h, hipMemcpyAsync(bs.h_fail, d.unit_fail, (size_t)nlp * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    for (i64 k = 0; k < nlp; ++k)
        if (bs.h_fail[k] != FAIL_NONE) { fail_col[k] = bs.h_fail[k]; ++*nfail; }
    return rc;
}

int tlpk_ipm_batch_skip(tlpk_handle *h, int on) {
    if (!h) return TLPK_BADARG;
    if (!ipm_is_batch(h)) { h->last_error = "tlpk_ipm_batch_skip: the handle is not batch-loaded (tlpk_ipm_load_batch)"; return TLPK_BADARG; }
    if (h->refine_steps > 0) { h->last_error = "tlpk_ipm_batch_skip: refine_steps > 0: the norms of the refinement run over all rows"; return TLPK_BADARG; }
    if (!on) { h->batch_skip = false; return TLPK_OK; }
    const IpmBatchState &bs = *h->ipm->bat;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = batch_unit_tables(h, bs, "tlpk_ipm_batch_skip")) return rc;
    if (int rc = skip_device_tables(h)) return rc;
    h->batch_skip = true;
    return TLPK_OK;
}

/* tlpk_ipm_hsolve_newton per LP: sc[8 k ..] and out[4 k ..] in its layouts; inactive LPs: out = 0 */
int tlpk_ipm_batch_hsolve_newton(tlpk_handle *h, const uint8_t *active, const double *sc, double *out) {
    IpmBatchState *bp = nullptr;
    if (int rc = batch_state(h, bp)) return rc;
    if (!active || !sc || !out) return TLPK_BADARG;
    IpmBatchState &bs = *bp; IpmState &s = *h->ipm; const i64 nlp = bs.nlp;
    const IpmDir &dst = s.D[s.cur];
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = batch_scalars(h, bs, active, [&](i64 k, int q) { return q < 3 ? sc[8 * k + 5 + q] : 0.0; })) return rc;      // eta, gamma mu, delta
    ipmb_launch_hrhs(h->stream, s.v, bs.B);
    ipmb_launch_newton_pre(h->stream, s.v, dst, bs.B, 0, bs.partials[0]);
    int rc;
    {
        MaskScope mask(h, bs);
        rc = mask.rc != TLPK_OK ? mask.rc : tlpk_solve2_device(h, bs.sx[0], bs.sy[0], s.v.b, s.v.hxid, bs.sx[1], bs.sy[1], s.v.xip, s.v.xid);
    }
    if (rc != TLPK_OK) return rc;
    ipmb_launch_take(h->stream, s.v.hx, s.v.hy, bs.sx[0], bs.sy[0], bs.B);      // an inactive LP keeps its h-system and direction
    ipmb_launch_take(h->stream, dst.x, dst.y, bs.sx[1], bs.sy[1], bs.B);
    ipmb_launch_hdots(h->stream, s.v, bs.B, bs.partials[1]);
    ipmb_launch_finalize(h->stream, bs.B, bs.B.tb, 2, 0, 0, bs.partials[1], bs.d_out + nlp * IPM_SLOTS);
    ipmb_launch_newton_dots(h->stream, s.v, dst, bs.B, bs.partials[0]);
    ipmb_launch_finalize(h->stream, bs.B, bs.B.tb, 6, 0, 0, bs.partials[0], bs.d_out);
    if ((rc = batch_gather(h, bs, 2)) != TLPK_OK) return rc;
    if ((rc = tlpk_sync(h)) != TLPK_OK) return rc;
    for (i64 k = 0; k < nlp; ++k) {
        double *o = out + 4 * k;
        o[0] = o[1] = o[2] = o[3] = 0.0;
        if (!active[k]) continue;
        const double *q = bs.h_out + (size_t)k * IPM_SLOTS, *qh = bs.h_out + (size_t)(nlp + k) * IPM_SLOTS, *c = sc + 8 * k;
        const double tau = c[0], kappa = c[1], regG = c[2];
        o[3] = ((qh[0] + qh[1]) + kappa / tau) + regG;                   // h0: the association of tlpk_ipm_hsolve_newton
        newton_scalars(q, tau, kappa, o[3], c[3], c[4], o[0], o[1]);
    }
    if ((rc = batch_scalars(h, bs, active, [&](i64 k, int q) { return q == 0 ? out[4 * k] : 0.0; })) != TLPK_OK) return rc;      // dtau
    ipmb_launch_newton_post(h->stream, s.v, dst, dst, bs.B, 0, bs.partials[1]);
    ipmb_launch_finalize(h->stream, bs.B, bs.B.tb, 0, 0, 2, bs.partials[1], bs.d_out);
    if ((rc = batch_gather(h, bs, 1)) != TLPK_OK) return rc;
    for (i64 k = 0; k < nlp; ++k) if (active[k]) { const double *q = bs.h_out + (size_t)k * IPM_SLOTS; out[4 * k + 2] = std::fmin(q[0], q[1]); }
    return TLPK_OK;
}

/* tlpk_ipm_newton per LP (one mode for the call): sc[8 k ..], out[3 k ..]; inactive LPs: out = 0 */
int tlpk_ipm_batch_newton(tlpk_handle *h, int mode, const uint8_t *active, const double *sc, double *out) {
    IpmBatchState *bp = nullptr;
    if (int rc = batch_state(h, bp)) return rc;
    if (!active || !sc || !out || mode < 0 || mode > 2) return TLPK_BADARG;
    IpmBatchState &bs = *bp; IpmState &s = *h->ipm; const i64 nlp = bs.nlp;
    const IpmDir &acc = s.D[s.cur];
    const IpmDir &dst = (mode == 2) ? s.D[1 - s.cur] : s.D[s.cur];
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = batch_scalars(h, bs, active, [&](i64 k, int q) { return q < 3 ? sc[8 * k + 5 + q] : 0.0; })) return rc;
    ipmb_launch_newton_pre(h->stream, s.v, acc, bs.B, mode, bs.partials[0]);
    int rc;
    {
        MaskScope mask(h, bs);
        rc = mask.rc != TLPK_OK ? mask.rc : tlpk_solve_device(h, bs.sx[0], bs.sy[0], s.v.xip, s.v.xid);
    }
    if (rc != TLPK_OK) return rc;
    ipmb_launch_take(h->stream, dst.x, dst.y, bs.sx[0], bs.sy[0], bs.B);        // an inactive LP keeps its direction
    ipmb_launch_newton_dots(h->stream, s.v, dst, bs.B, bs.partials[0]);
    ipmb_launch_finalize(h->stream, bs.B, bs.B.tb, 6, 0, 0, bs.partials[0], bs.d_out);
    if ((rc = batch_gather(h, bs, 1)) != TLPK_OK) return rc;
    if ((rc = tlpk_sync(h)) != TLPK_OK) return rc;
    for (i64 k = 0; k < nlp; ++k) {
        double *o = out + 3 * k;
        o[0] = o[1] = o[2] = 0.0;
        if (!active[k]) continue;
        const double *c = sc + 8 * k;
        newton_scalars(bs.h_out + (size_t)k * IPM_SLOTS, c[0], c[1], c[2], c[3], c[4], o[0], o[1]);
    }
    if ((rc = batch_scalars(h, bs, active, [&](i64 k, int q) { return q == 0 ? out[3 * k] : 0.0; })) != TLPK_OK) return rc;
    ipmb_launch_newton_post(h->stream, s.v, dst, acc, bs.B, mode == 2 ? 1 : 0, bs.partials[1]);
    ipmb_launch_finalize(h->stream, bs.B, bs.B.tb, 0, 0, 2, bs.partials[1], bs.d_out);
    if ((rc = batch_gather(h, bs, 1)) != TLPK_OK) return rc;
    for (i64 k = 0; k < nlp; ++k) if (active[k]) { const double *q = bs.h_out + (size_t)k * IPM_SLOTS; out[3 * k + 2] = std::fmin(q[0], q[1]); }
    return TLPK_OK;
}

/* tlpk_ipm_targets per LP: par[3 k ..] = { a_, mu_l, mu_u }, out[2 k ..] = { sum(vl), sum(vu) } */
int tlpk_ipm_batch_targets(tlpk_handle *h, const uint8_t *active, const double *par, double *out) {
    IpmBatchState *bp = nullptr;
    if (int rc = batch_state(h, bp)) return rc;
    if (!active || !par || !out) return TLPK_BADARG;
    IpmBatchState &bs = *bp; IpmState &s = *h->ipm;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = batch_scalars(h, bs, active, [&](i64 k, int q) { return q < 3 ? par[3 * k + q] : 0.0; })) return rc;
    ipmb_launch_targets(h->stream, s.v, s.D[s.cur], bs.B, bs.partials[0]);
    ipmb_launch_finalize(h->stream, bs.B, bs.B.tc, 2, 0, 0, bs.partials[0], bs.d_out);
    if (int rc = batch_gather(h, bs, 1)) return rc;
    for (i64 k = 0; k < bs.nlp; ++k) { const double *q = bs.h_out + (size_t)k * IPM_SLOTS; out[2 * k] = q[0]; out[2 * k + 1] = q[1]; }
    return TLPK_OK;
}

/* tlpk_ipm_accept for the LPs with active[k] != 0: their candidate of the last mode-2 call becomes their accepted direction */
int tlpk_ipm_batch_accept(tlpk_handle *h, const uint8_t *active) {
    IpmBatchState *bp = nullptr;
    if (int rc = batch_state(h, bp)) return rc;
    if (!active) return TLPK_BADARG;
    IpmBatchState &bs = *bp; IpmState &s = *h->ipm;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = batch_scalars(h, bs, active, [](i64, int) { return 0.0; })) return rc;
    ipmb_launch_accept(h->stream, s.D[s.cur], s.D[1 - s.cur], bs.B);
    HIPCHK(h, hipStreamSynchronize(h->stream));                      // the next call rewrites the pinned scalars
    HIPCHK(h, hipGetLastError());
    return TLPK_OK;
}

/* tlpk_ipm_advance per LP: pt_k += alpha[k] D_k; out[k] = xl'zl + xu'zu of the new point (0 for an inactive LP, which is not moved) */
int tlpk_ipm_batch_advance(tlpk_handle *h, const uint8_t *active, const double *alpha, double *out) {
    IpmBatchState *bp = nullptr;
    if (int rc = batch_state(h, bp)) return rc;
    if (!active || !alpha || !out) return TLPK_BADARG;
    IpmBatchState &bs = *bp; IpmState &s = *h->ipm;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = batch_scalars(h, bs, active, [&](i64 k, int q) { return q == 0 ? alpha[k] : 0.0; })) return rc;
    ipmb_launch_advance(h->stream, s.v, s.D[s.cur], bs.B, bs.partials[0]);
    ipmb_launch_finalize(h->stream, bs.B, bs.B.tb, 1, 0, 0, bs.partials[0], bs.d_out);
    if (int rc = batch_gather(h, bs, 1)) return rc;
    for (i64 k = 0; k < bs.nlp; ++k) out[k] = bs.h_out[(size_t)k * IPM_SLOTS];
    return TLPK_OK;
}

/* ---- a batch that keeps going (include/tlpk.h, "Refilling slots"; DESIGN.md section 4b'-r) -------------------------------------------------
 * tlpk_ipm_batch_refill gives the slots with slots[k] != 0 a new LP on the analysed pattern: tlpk_set_values + tlpk_ipm_reload restricted to those
 * LPs.  Every other LP keeps every bit of its state.  tlpk_ipm_get_lp reads one LP's segment of a vector (the result of an LP that leaves). */
}  // extern "C"

namespace {

// first refill with new values: where every LP's entries sit in the caller's nzval.  The stacked matrix is block diagonal in the caller's column-major order, so LP k owns
// the contiguous range [nz_off[k], nz_off[k + 1]); that is verified here, entry by entry.  K2: the map of the loops' row-major copy of A (ipm_sub_matrix's order).
int refill_maps(tlpk_handle *h, IpmBatchState &bs) {
    if (bs.refill_maps) return TLPK_OK;
    if (int rc = sync_host_values(h)) return rc;
    const Symbolic &S = h->S;
    const bool k2 = S.system == 1;
    const i64 nnz = k2 ? S.n : S.nnzA, nlp = bs.nlp;
    std::vector<i32> lp_of((size_t)nnz);
    bs.nz_off.assign((size_t)nlp + 1, 0);
    auto lp_of_col = [&](i64 j) { return (i64)(std::upper_bound(bs.col_off.begin(), bs.col_off.end(), j) - bs.col_off.begin()) - 1; };
    if (!k2) {
        for (i64 j = 0; j < S.n; ++j) { const i64 k = lp_of_col(j); for (i64 p = S.Ap[(size_t)j]; p < S.Ap[(size_t)j + 1]; ++p) lp_of[(size_t)p] = (i32)k; }
    } else {
        for (i64 p = 0; p < nnz; ++p) { const i64 q = S.Ap[(size_t)p]; lp_of[(size_t)p] = (i32)lp_of_col(std::min(S.Ai[(size_t)q], S.Ai[(size_t)q + 1])); }
    }
    for (i64 p = 0; p < nnz; ++p) {
        const i64 k = lp_of[(size_t)p];
        if (k < 0 || k >= nlp || (p > 0 && k < lp_of[(size_t)p - 1])) { h->last_error = "tlpk_ipm_batch_refill: the entries of an LP are not a contiguous range of nzval"; return TLPK_INTERNAL; }
        ++bs.nz_off[(size_t)k + 1];
    }
    for (i64 k = 0; k < nlp; ++k) bs.nz_off[(size_t)k + 1] += bs.nz_off[(size_t)k];
    i32 *di;
    if (int rc = dev_upload(h, &di, lp_of)) return rc;
    bs.d_lp_of = di;
    if (k2) {
        std::vector<i64> ap, tp; std::vector<i32> ai, tj, src; std::vector<double> ax, tx;
        if (int rc = ipm_sub_matrix(h, false, ap, ai, ax, tp, tj, tx)) return rc;
        if ((i64)ai.size() != nnz) { h->last_error = "tlpk_ipm_batch_refill: the loops' copy of A does not match nzval"; return TLPK_INTERNAL; }
        src.resize(ai.size());
        std::vector<i64> cur(tp.begin(), tp.end() - 1);
        for (size_t q = 0; q < ai.size(); ++q) src[(size_t)cur[(size_t)ai[q]]++] = (i32)q;      // the order in which ipm_sub_matrix fills tx
        if (int rc = dev_upload(h, &di, src)) return rc;
        bs.d_ktx_src = di;
    }
    bs.refill_maps = true;
    return TLPK_OK;
}

}  // namespace

extern "C" {

int tlpk_ipm_batch_refill(tlpk_handle *h, const uint8_t *slots, const double *nzval, int64_t len,
                          const double *b, const double *c, const double *l, const double *u) {
    if (!h) return TLPK_BADARG;
    if (!h->ipm) { h->last_error = "tlpk_ipm_load_batch has not been called (load first)"; return TLPK_BADARG; }
    if (!h->ipm->bat) { h->last_error = "the handle holds one LP (tlpk_ipm_load): the tlpk_ipm_batch_* calls need tlpk_ipm_load_batch"; return TLPK_BADARG; }
    if (!slots) { h->last_error = "tlpk_ipm_batch_refill: slots is NULL"; return TLPK_BADARG; }
    const Symbolic &S = h->S;
    const bool k2 = S.system == 1;
    const i64 nnz = k2 ? S.n : S.nnzA;
    if (nzval && len != nnz) { h->last_error = "tlpk_ipm_batch_refill: len = " + std::to_string(len) + ", the analysed matrix has " + std::to_string(nnz) + " entries"; return TLPK_BADARG; }
    IpmBatchState *bp = nullptr;
    if (int rc = batch_state(h, bp)) return rc;                       // (the stale handle; an analyse-only handle is never loaded)
    IpmBatchState &bs = *bp; IpmState &s = *h->ipm; const IpmVecs &v = s.v; const i64 nlp = bs.nlp;
    // runs of selected slots: neighbours share their copies
    std::vector<i64> runs;
    for (i64 k = 0; k < nlp; ++k) {
        if (!slots[k]) continue;
        if (!runs.empty() && runs.back() == k) runs.back() = k + 1;
        else { runs.push_back(k); runs.push_back(k + 1); }
    }
    if (runs.empty()) return TLPK_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));                       // nothing of the previous call reads the vectors or the pinned scalars any more
    if (nzval) if (int rc = refill_maps(h, bs)) return rc;
    if (int rc = batch_scalars(h, bs, slots, [](i64, int) { return 0.0; })) return rc;      // the flags: what the kernels below select by
    hipStream_t st = h->stream;
    if (nzval) {
        std::vector<i64> ranges;
        for (size_t r = 0; r < runs.size(); r += 2) { ranges.push_back(bs.nz_off[(size_t)runs[r]]); ranges.push_back(bs.nz_off[(size_t)runs[r + 1]]); }
        if (int rc = set_values_slots(h, nzval, ranges, bs.d_lp_of, bs.d_sc + (IPM_BSC - 1), IPM_BSC)) return rc;
        if (k2) {
            // the loops' own copies: column-major = nzval's order, row-major through its map
            for (size_t r = 0; r < ranges.size(); r += 2)
                if (ranges[r + 1] > ranges[r]) HIPCHK(h, hipMemcpyAsync(const_cast<double *>(v.Ax) + ranges[r], nzval + ranges[r], (size_t)(ranges[r + 1] - ranges[r]) * 8, hipMemcpyHostToDevice, st));
            launch_refresh_gather_sel(st, nnz, bs.d_ktx_src, h->d_nz, const_cast<double *>(v.Tx), bs.d_lp_of, bs.d_sc + (IPM_BSC - 1), IPM_BSC);
        }
    }
    // the vectors: the selected segments; flag and bound .* flag as tlpk_ipm_load forms them (ipmdata.jl:46-47).  The staging lives until the wait below.
    std::vector<double> stage;
    if (l || u) {
        i64 total = 0;
        for (size_t r = 0; r < runs.size(); r += 2) total += bs.col_off[(size_t)runs[r + 1]] - bs.col_off[(size_t)runs[r]];
        stage.resize((size_t)(4 * total));
    }
    double *sp = stage.data();
    for (size_t r = 0; r < runs.size(); r += 2) {
        const i64 r0 = bs.row_off[(size_t)runs[r]], mk = bs.row_off[(size_t)runs[r + 1]] - r0;
        const i64 c0 = bs.col_off[(size_t)runs[r]], nk = bs.col_off[(size_t)runs[r + 1]] - c0;
        if (b) HIPCHK(h, hipMemcpyAsync(const_cast<double *>(v.b) + r0, b + r0, (size_t)mk * 8, hipMemcpyHostToDevice, st));
        if (c) HIPCHK(h, hipMemcpyAsync(const_cast<double *>(v.c) + c0, c + c0, (size_t)nk * 8, hipMemcpyHostToDevice, st));
        for (int side = 0; side < 2; ++side) {
            const double *bd = side ? u : l;
            if (!bd) continue;
            double *w0 = sp, *w1 = sp + nk;
            sp += 2 * nk;
            for (i64 j = 0; j < nk; ++j) { const bool f = std::isfinite(bd[c0 + j]); w0[j] = f ? 1.0 : 0.0; w1[j] = f ? bd[c0 + j] : 0.0; }
            HIPCHK(h, hipMemcpyAsync(const_cast<double *>(side ? v.uflag : v.lflag) + c0, w0, (size_t)nk * 8, hipMemcpyHostToDevice, st));
            HIPCHK(h, hipMemcpyAsync(const_cast<double *>(side ? v.uz : v.lz) + c0, w1, (size_t)nk * 8, hipMemcpyHostToDevice, st));
        }
    }
    ipmb_launch_init(st, v, bs.B);                                    // HSD.jl:238-247 on the selected LPs
    HIPCHK(h, hipStreamSynchronize(st));
    HIPCHK(h, hipGetLastError());
    return TLPK_OK;
}

int tlpk_ipm_get_lp(tlpk_handle *h, int what, int64_t k, double *host, int64_t len) {
    Shards sh;
    if (int rc = ipm_shards(h, sh, true, true, true)) return rc;
    if (!host || what < 0 || what > 35) return TLPK_BADARG;
    IpmBatchState *bs = h->ipm->bat;
    if (!bs) { h->last_error = "tlpk_ipm_get_lp: the handle holds one LP (tlpk_ipm_load): it needs tlpk_ipm_load_batch"; return TLPK_BADARG; }
    if (k < 0 || k >= bs->nlp) { h->last_error = "tlpk_ipm_get_lp: LP " + std::to_string(k) + " of " + std::to_string(bs->nlp); return TLPK_BADARG; }
    const std::vector<i64> &off = ipm_get_is_row(what) ? bs->row_off : bs->col_off;
    const i64 need = off[(size_t)k + 1] - off[(size_t)k];
    if (len != need) { h->last_error = "tlpk_ipm_get_lp: wrong length"; return TLPK_BADARG; }
    const double *src[36];
    ipm_get_sources(h, src);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!src[what]) { h->last_error = "tlpk_ipm_get_lp: the handle does not hold that vector"; return TLPK_BADARG; }
    HIPCHK(h, hipMemcpy(host, src[what] + off[(size_t)k], (size_t)need * 8, hipMemcpyDeviceToHost));
    return TLPK_OK;
}

/* ---- Mehrotra predictor-corrector on a stack of LPs (include/tlpk.h, "Batched device-resident MPC"; DESIGN.md section 4b'') -------------
 * The tlpk_mpc_* calls with per-LP scalars and `active` masks.  tlpk_ipm_batch_residuals (tau[k] = 1), tlpk_ipm_batch_factor and
 * tlpk_ipm_batch_accept are shared with the HSD batch as they are. */

/* tlpk_mpc_start per LP, stage by stage (every LP is active): out[k] = xl'zl + xu'zu of LP k's starting point */
int tlpk_mpc_batch_start(tlpk_handle *h, double *out) {
    IpmBatchState *bp = nullptr;
    if (int rc = batch_state(h, bp)) return rc;
    if (!out) { h->last_error = "tlpk_mpc_batch_start: a NULL pointer"; return TLPK_BADARG; }
    IpmBatchState &bs = *bp; IpmState &s = *h->ipm; const i64 nlp = bs.nlp;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = batch_scalars(h, bs, nullptr, [](i64, int) { return 0.0; })) return rc;
    mpcb_launch_fill(h->stream, s.v, bs.B, h->d_theta, h->d_regP, h->d_regD);
    int rc = tlpk_update_device(h, h->d_theta, h->d_regP, h->d_regD);
    if (rc != TLPK_OK) return rc;
    if ((rc = tlpk_solve_device(h, s.D[0].x, s.v.y, s.v.xip, s.v.c)) != TLPK_OK) return rc;      // y  (xip == 0 here)
    if ((rc = tlpk_solve_device(h, s.v.x, s.D[0].y, s.v.b, s.v.xid)) != TLPK_OK) return rc;      // x  (xid == 0 here)
    const double *q = bs.h_out;
    // one stage: the scalars sc(k, slot) of every LP, the kernel, the per-LP reductions
    auto stage = [&](int st, auto &&sc, int nsum, int nmin) -> int {
        if (st > 1) if (int r = batch_scalars(h, bs, nullptr, sc)) return r;
        mpcb_launch_start(h->stream, s.v, bs.B, st, bs.partials[0]);
        ipmb_launch_finalize(h->stream, bs.B, bs.B.tc, nsum, 0, nmin, bs.partials[0], bs.d_out);
        return batch_gather(h, bs, 1);
    };
    std::vector<double> a((size_t)nlp), b((size_t)nlp);
    if ((rc = stage(1, [](i64, int) { return 0.0; }, 0, 2)) != TLPK_OK) return rc;
    if ((rc = tlpk_sync(h)) != TLPK_OK) return rc;
    for (i64 k = 0; k < nlp; ++k) { const double *r = q + (size_t)k * IPM_SLOTS; a[(size_t)k] = 1.0 + std::fmax(0.0, std::fmax(-1.5 * r[0], -1.5 * r[1])); }      // dxs
    if ((rc = stage(2, [&](i64 k, int slot) { return slot == 0 ? a[(size_t)k] : 0.0; }, 0, 2)) != TLPK_OK) return rc;
    for (i64 k = 0; k < nlp; ++k) { const double *r = q + (size_t)k * IPM_SLOTS; a[(size_t)k] = 1.0 + std::fmax(0.0, std::fmax(-1.5 * r[0], -1.5 * r[1])); }      // dzs
    if ((rc = stage(3, [&](i64 k, int slot) { return slot == 0 ? a[(size_t)k] : 0.0; }, 3, 0)) != TLPK_OK) return rc;
    for (i64 k = 0; k < nlp; ++k) {
        const double *r = q + (size_t)k * IPM_SLOTS;
        const double mu = r[0];
        a[(size_t)k] = mu / (2.0 * r[1]); b[(size_t)k] = mu / (2.0 * r[2]);      // ddx, ddz
    }
    if ((rc = stage(4, [&](i64 k, int slot) { return slot == 0 ? a[(size_t)k] : (slot == 1 ? b[(size_t)k] : 0.0); }, 1, 0)) != TLPK_OK) return rc;
    for (i64 k = 0; k < nlp; ++k) out[k] = q[(size_t)k * IPM_SLOTS];
    s.cur = 0;
    return TLPK_OK;
}

/* tlpk_mpc_newton per LP (one mode for the call): gmu[k]; out[2 k ..] = { primal, dual step to the boundary }; inactive LPs: out = 0 */
int tlpk_mpc_batch_newton(tlpk_handle *h, int mode, const uint8_t *active, const double *gmu, double *out) {
    IpmBatchState *bp = nullptr;
    if (int rc = batch_state(h, bp)) return rc;
    if (!active || !gmu || !out) { h->last_error = "tlpk_mpc_batch_newton: a NULL pointer"; return TLPK_BADARG; }
    if (mode < 0 || mode > 2) { h->last_error = "tlpk_mpc_batch_newton: mode must be 0, 1 or 2"; return TLPK_BADARG; }
    IpmBatchState &bs = *bp; IpmState &s = *h->ipm; const i64 nlp = bs.nlp;
    const IpmDir &acc = s.D[s.cur];
    const IpmDir &dst = (mode == 2) ? s.D[1 - s.cur] : s.D[s.cur];
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = batch_scalars(h, bs, active, [&](i64 k, int q) { return q == 0 ? 1.0 : (q == 1 ? gmu[k] : 0.0); })) return rc;      // eta = 1, gamma mu, delta = 0
    ipmb_launch_newton_pre(h->stream, s.v, acc, bs.B, mode, bs.partials[0]);
    int rc;
    {
        MaskScope mask(h, bs);
        rc = mask.rc != TLPK_OK ? mask.rc : tlpk_solve_device(h, bs.sx[0], bs.sy[0], s.v.xip, s.v.xid);
    }
    if (rc != TLPK_OK) return rc;
    ipmb_launch_take(h->stream, dst.x, dst.y, bs.sx[0], bs.sy[0], bs.B);        // an inactive LP keeps its direction
    if ((rc = tlpk_sync(h)) != TLPK_OK) return rc;                              // the kernels above have read this call's first scalars
    if ((rc = batch_scalars(h, bs, active, [](i64, int) { return 0.0; })) != TLPK_OK) return rc;      // dtau = 0: hx, hy (zeros) unused
    ipmb_launch_newton_post(h->stream, s.v, dst, acc, bs.B, mode == 2 ? 1 : 0, bs.partials[1]);
    ipmb_launch_finalize(h->stream, bs.B, bs.B.tb, 0, 0, 2, bs.partials[1], bs.d_out);
    if ((rc = batch_gather(h, bs, 1)) != TLPK_OK) return rc;
    for (i64 k = 0; k < nlp; ++k) { const double *q = bs.h_out + (size_t)k * IPM_SLOTS; out[2 * k] = q[0]; out[2 * k + 1] = q[1]; }
    return TLPK_OK;
}

/* tlpk_mpc_gap per LP: out[2 k ..] = { complementarity of LP k moved by (ap[k], ad[k]) along its accepted direction, at the point itself } */
int tlpk_mpc_batch_gap(tlpk_handle *h, const uint8_t *active, const double *ap, const double *ad, double *out) {
    IpmBatchState *bp = nullptr;
    if (int rc = batch_state(h, bp)) return rc;
    if (!active || !ap || !ad || !out) { h->last_error = "tlpk_mpc_batch_gap: a NULL pointer"; return TLPK_BADARG; }
    IpmBatchState &bs = *bp; IpmState &s = *h->ipm;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = batch_scalars(h, bs, active, [&](i64 k, int q) { return q == 0 ? ap[k] : (q == 1 ? ad[k] : 0.0); })) return rc;
    mpcb_launch_gap(h->stream, s.v, s.D[s.cur], bs.B, bs.partials[0]);
    ipmb_launch_finalize(h->stream, bs.B, bs.B.tc, 2, 0, 0, bs.partials[0], bs.d_out);
    if (int rc = batch_gather(h, bs, 1)) return rc;
    for (i64 k = 0; k < bs.nlp; ++k) { const double *q = bs.h_out + (size_t)k * IPM_SLOTS; out[2 * k] = q[0]; out[2 * k + 1] = q[1]; }
    return TLPK_OK;
}

/* tlpk_mpc_targets per LP: par[4 k ..] = { ap_, ad_, tmin, tmax }; the targets stay on the device for tlpk_mpc_batch_newton(mode 2) */
int tlpk_mpc_batch_targets(tlpk_handle *h, const uint8_t *active, const double *par) {
    IpmBatchState *bp = nullptr;
    if (int rc = batch_state(h, bp)) return rc;
    if (!active || !par) { h->last_error = "tlpk_mpc_batch_targets: a NULL pointer"; return TLPK_BADARG; }
    IpmBatchState &bs = *bp; IpmState &s = *h->ipm;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = batch_scalars(h, bs, active, [&](i64 k, int q) { return q < 4 ? par[4 * k + q] : 0.0; })) return rc;
    mpcb_launch_targets(h->stream, s.v, s.D[s.cur], bs.B, bs.partials[0]);
    HIPCHK(h, hipStreamSynchronize(h->stream));                      // the next call rewrites the pinned scalars
    HIPCHK(h, hipGetLastError());
    return TLPK_OK;
}

/* tlpk_mpc_advance per LP: primal side += ap[k] D_k, dual side += ad[k] D_k; out[k] = xl'zl + xu'zu of the new point (0 for an inactive LP) */
int tlpk_mpc_batch_advance(tlpk_handle *h, const uint8_t *active, const double *ap, const double *ad, double *out) {
    IpmBatchState *bp = nullptr;
    if (int rc = batch_state(h, bp)) return rc;
    if (!active || !ap || !ad || !out) { h->last_error = "tlpk_mpc_batch_advance: a NULL pointer"; return TLPK_BADARG; }
    IpmBatchState &bs = *bp; IpmState &s = *h->ipm;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = batch_scalars(h, bs, active, [&](i64 k, int q) { return q == 0 ? ap[k] : (q == 1 ? ad[k] : 0.0); })) return rc;
    mpcb_launch_advance(h->stream, s.v, s.D[s.cur], bs.B, bs.partials[0]);
    ipmb_launch_finalize(h->stream, bs.B, bs.B.tb, 1, 0, 0, bs.partials[0], bs.d_out);
    if (int rc = batch_gather(h, bs, 1)) return rc;
    for (i64 k = 0; k < bs.nlp; ++k) out[k] = bs.h_out[(size_t)k * IPM_SLOTS];
    return TLPK_OK;
}

/* ---- the Mehrotra stream (include/tlpk.h, "Entering LPs"; DESIGN.md section 4b''-s) ---------------------------------------------------------
 * An LP that enters a slot needs the starting point of tlpk_mpc_batch_start: one factorisation and two solves.  A stacked update factorises every
 * block with that block's own values and a stacked solve takes a right-hand side per block, so the entering LP rides in the update and in the
 * predictor and corrector solves of the running LPs: the calls below are tlpk_ipm_batch_factor / tlpk_mpc_batch_newton with an `enter` mask beside
 * `active`.  Only the column kernels of the starting point (tlpk_mpc_batch_enter_finish) are launches of the entering LPs' own. */
}  // extern "C"

namespace {

// the refusals of the three calls in their order: not loaded / not batch-loaded, NULL pointers, the stale handle, an LP with two roles, no device
int enter_state(tlpk_handle *h, IpmBatchState *&bs, const char *name, bool null_ptr, const uint8_t *active, const uint8_t *enter) {
    if (!h) return TLPK_BADARG;
    if (!h->ipm) { h->last_error = "tlpk_ipm_load_batch has not been called (load first)"; return TLPK_BADARG; }
    if (!h->ipm->bat) { h->last_error = "the handle holds one LP (tlpk_ipm_load): the tlpk_ipm_batch_* calls need tlpk_ipm_load_batch"; return TLPK_BADARG; }
    if (null_ptr) { h->last_error = std::string(name) + ": a NULL pointer"; return TLPK_BADARG; }
    if (h->ipm_stale) {
        h->last_error = "the matrix values changed (tlpk_set_values) after the LPs were loaded: call tlpk_ipm_reload before the device-resident loops";
        return TLPK_BADARG;
    }
    bs = h->ipm->bat;
    if (active)
        for (i64 k = 0; k < bs->nlp; ++k)
            if (active[k] && enter[k]) { h->last_error = std::string(name) + ": LP " + std::to_string(k) + " is both active and entering"; return TLPK_BADARG; }
    if (!h->has_device) return TLPK_NO_DEVICE;
    return TLPK_OK;
}
// batch_scalars with the roles: sc(k, q) for q < IPM_ROLE, the role, the `active` flag (0 for an entering LP: the kernels of the running LPs skip it)
template <class F>
int role_scalars(tlpk_handle *h, IpmBatchState &bs, const uint8_t *active, const uint8_t *enter, F &&sc) {
    for (i64 k = 0; k < bs.nlp; ++k) {
        double *row = bs.h_sc + (size_t)k * IPM_BSC;
        for (int q = 0; q < IPM_ROLE; ++q) row[q] = sc(k, q);
        row[IPM_ROLE] = active[k] ? IPM_ACTIVE : (enter[k] ? IPM_ENTERING : IPM_PARKED);
        row[IPM_BSC - 1] = active[k] ? 1.0 : 0.0;
    }
    HIPCHK(h, hipMemcpyAsync(bs.d_sc, bs.h_sc, (size_t)bs.nlp * IPM_BSC * 8, hipMemcpyHostToDevice, h->stream));
    return TLPK_OK;
}
bool any_of(const uint8_t *mask, i64 n) { for (i64 k = 0; k < n; ++k) if (mask[k]) return true; return false; }

}  // namespace

extern "C" {

/* tlpk_ipm_batch_factor with three roles: active (regP[k], regD[k]), entering (the starting matrix: theta_inv = 0, Rp = 1, Rd = 1e-6), parked */
int tlpk_mpc_batch_factor_enter(tlpk_handle *h, const uint8_t *active, const uint8_t *enter, const double *regP, const double *regD, int64_t *fail_lp) {
    IpmBatchState *bp = nullptr;
    if (int rc = enter_state(h, bp, "tlpk_mpc_batch_factor_enter", !active || !enter || !regP || !regD || !fail_lp, active, enter)) return rc;
    IpmBatchState &bs = *bp;
    *fail_lp = -1;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = role_scalars(h, bs, active, enter, [&](i64 k, int q) { return q == 0 ? regP[k] : (q == 1 ? regD[k] : 0.0); })) return rc;
    mpcb_launch_theta_enter(h->stream, h->ipm->v, bs.B, h->d_theta, h->d_regP, h->d_regD);
    MaskScope mask(h, bs, IPM_ROLE);                                  // parked = neither active nor entering
    if (mask.rc != TLPK_OK) return mask.rc;
    const int rc = tlpk_update_device(h, h->d_theta, h->d_regP, h->d_regD);
    if (rc == TLPK_NOT_POSDEF) *fail_lp = batch_owner(h, bs, h->fail_col);
    return rc;
}

/* tlpk_mpc_batch_newton(mode 0 | 1) for the active LPs; the entering LPs take one of the two solves of their starting point from the same stacked solve */
int tlpk_mpc_batch_newton_enter(tlpk_handle *h, int mode, const uint8_t *active, const uint8_t *enter, const double *gmu, double *out) {
    IpmBatchState *bp = nullptr;
    if (int rc = enter_state(h, bp, "tlpk_mpc_batch_newton_enter", !active || !enter || !gmu || !out, active, enter)) return rc;
    if (mode < 0 || mode > 1) { h->last_error = "tlpk_mpc_batch_newton_enter: mode must be 0 or 1 (the centrality correctors go through tlpk_mpc_batch_newton)"; return TLPK_BADARG; }
    IpmBatchState &bs = *bp; IpmState &s = *h->ipm; const i64 nlp = bs.nlp;
    const IpmDir &acc = s.D[s.cur];
    const bool entering = any_of(enter, nlp);
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = role_scalars(h, bs, active, enter, [&](i64 k, int q) { return q == 0 ? 1.0 : (q == 1 ? gmu[k] : 0.0); })) return rc;      // eta = 1, gamma mu, delta = 0
    ipmb_launch_newton_pre(h->stream, s.v, acc, bs.B, mode, bs.partials[0]);
    if (entering) mpcb_launch_enter_rhs(h->stream, s.v, bs.B, mode);
    int rc;
    {
        MaskScope mask(h, bs, IPM_ROLE);
        rc = mask.rc != TLPK_OK ? mask.rc : tlpk_solve_device(h, bs.sx[0], bs.sy[0], s.v.xip, s.v.xid);
    }
    if (rc != TLPK_OK) return rc;
    ipmb_launch_take(h->stream, acc.x, acc.y, bs.sx[0], bs.sy[0], bs.B);
    if (entering) mpcb_launch_enter_take(h->stream, s.v, s.D[0], bs.sx[0], bs.sy[0], bs.B, mode);      // D[0]: where tlpk_mpc_batch_start keeps its two halves
    if ((rc = tlpk_sync(h)) != TLPK_OK) return rc;                              // the kernels above have read this call's first scalars
    if ((rc = batch_scalars(h, bs, active, [](i64, int) { return 0.0; })) != TLPK_OK) return rc;      // dtau = 0
    ipmb_launch_newton_post(h->stream, s.v, acc, acc, bs.B, 0, bs.partials[1]);
    ipmb_launch_finalize(h->stream, bs.B, bs.B.tb, 0, 0, 2, bs.partials[1], bs.d_out);
    if ((rc = batch_gather(h, bs, 1)) != TLPK_OK) return rc;
    for (i64 k = 0; k < nlp; ++k) { const double *q = bs.h_out + (size_t)k * IPM_SLOTS; out[2 * k] = q[0]; out[2 * k + 1] = q[1]; }
    return TLPK_OK;
}

/* stages 1 - 4 of tlpk_mpc_batch_start for the entering LPs, whose x, y and the halves in D[0] the two newton_enter calls have written */
int tlpk_mpc_batch_enter_finish(tlpk_handle *h, const uint8_t *enter, double *out) {
    IpmBatchState *bp = nullptr;
    if (int rc = enter_state(h, bp, "tlpk_mpc_batch_enter_finish", !enter || !out, nullptr, enter)) return rc;
    IpmBatchState &bs = *bp; IpmState &s = *h->ipm; const i64 nlp = bs.nlp;
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    const double *q = bs.h_out;
    // one stage: the kernels select by the flag, which here is `enter`
    auto stage = [&](int st, auto &&sc, int nsum, int nmin) -> int {
        if (int r = batch_scalars(h, bs, enter, sc)) return r;
        mpcb_launch_start(h->stream, s.v, bs.B, st, bs.partials[0]);
        ipmb_launch_finalize(h->stream, bs.B, bs.B.tc, nsum, 0, nmin, bs.partials[0], bs.d_out);
        return batch_gather(h, bs, 1);
    };
    std::vector<double> a((size_t)nlp), b((size_t)nlp);
    if ((rc = stage(1, [](i64, int) { return 0.0; }, 0, 2)) != TLPK_OK) return rc;
    if ((rc = tlpk_sync(h)) != TLPK_OK) return rc;
    for (i64 k = 0; k < nlp; ++k) { const double *r = q + (size_t)k * IPM_SLOTS; a[(size_t)k] = 1.0 + std::fmax(0.0, std::fmax(-1.5 * r[0], -1.5 * r[1])); }      // dxs
    if ((rc = stage(2, [&](i64 k, int slot) { return slot == 0 ? a[(size_t)k] : 0.0; }, 0, 2)) != TLPK_OK) return rc;
    for (i64 k = 0; k < nlp; ++k) { const double *r = q + (size_t)k * IPM_SLOTS; a[(size_t)k] = 1.0 + std::fmax(0.0, std::fmax(-1.5 * r[0], -1.5 * r[1])); }      // dzs
    if ((rc = stage(3, [&](i64 k, int slot) { return slot == 0 ? a[(size_t)k] : 0.0; }, 3, 0)) != TLPK_OK) return rc;
    for (i64 k = 0; k < nlp; ++k) {
        const double *r = q + (size_t)k * IPM_SLOTS;
        const double mu = r[0];
        a[(size_t)k] = mu / (2.0 * r[1]); b[(size_t)k] = mu / (2.0 * r[2]);      // ddx, ddz
    }
    if ((rc = stage(4, [&](i64 k, int slot) { return slot == 0 ? a[(size_t)k] : (slot == 1 ? b[(size_t)k] : 0.0); }, 1, 0)) != TLPK_OK) return rc;
    for (i64 k = 0; k < nlp; ++k) out[k] = enter[k] ? q[(size_t)k * IPM_SLOTS] : 0.0;
    return TLPK_OK;
}

/* tlpk_ipm_get_lp for several codes and several LPs: one gather kernel into a staging buffer, one copy out.  host: LP-major, the codes in the given order */
int tlpk_ipm_get_lps(tlpk_handle *h, const int32_t *what, int64_t nwhat, const int64_t *lp, int64_t nk, double *host, int64_t len) {
    Shards sh;
    if (int rc = ipm_shards(h, sh, true, true, true)) return rc;
    if (!host || !what || !lp || nwhat < 0 || nk < 0) return TLPK_BADARG;
    for (i64 w = 0; w < nwhat; ++w) if (what[w] < 0 || what[w] > 35) return TLPK_BADARG;
    IpmBatchState *bs = h->ipm->bat;
    if (!bs) { h->last_error = "tlpk_ipm_get_lps: the handle holds one LP (tlpk_ipm_load): it needs tlpk_ipm_load_batch"; return TLPK_BADARG; }
    std::vector<char> seen((size_t)bs->nlp, 0);
    i64 need = 0, maxlen = 0;
    for (i64 q = 0; q < nk; ++q) {
        const i64 k = lp[q];
        if (k < 0 || k >= bs->nlp) { h->last_error = "tlpk_ipm_get_lps: LP " + std::to_string(k) + " of " + std::to_string(bs->nlp); return TLPK_BADARG; }
        if (seen[(size_t)k]) { h->last_error = "tlpk_ipm_get_lps: LP " + std::to_string(k) + " is listed twice"; return TLPK_BADARG; }
        seen[(size_t)k] = 1;
        for (i64 w = 0; w < nwhat; ++w) {
            const std::vector<i64> &off = ipm_get_is_row(what[w]) ? bs->row_off : bs->col_off;
            const i64 seg = off[(size_t)k + 1] - off[(size_t)k];
            need += seg; maxlen = std::max(maxlen, seg);
        }
    }
    if (len != need) { h->last_error = "tlpk_ipm_get_lps: wrong length (the listed segments hold " + std::to_string(need) + " entries)"; return TLPK_BADARG; }
    const double *src[36];
    ipm_get_sources(h, src);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (i64 w = 0; w < nwhat; ++w) if (!src[what[w]]) { h->last_error = "tlpk_ipm_get_lps: the handle does not hold that vector"; return TLPK_BADARG; }
    const i64 nseg = nk * nwhat;
    if (nseg == 0 || need == 0) return TLPK_OK;
    if (nseg > ((i64)1 << 30)) { h->last_error = "tlpk_ipm_get_lps: too many segments"; return TLPK_TOO_LARGE; }
    if (nseg > bs->tab_cap) {
        if (bs->h_tab) { hipHostFree(bs->h_tab); bs->h_tab = nullptr; }
        if (bs->d_tab) { hipFree(bs->d_tab); bs->d_tab = nullptr; }
        bs->tab_cap = 0;
        const i64 cap = std::max<i64>(nseg, std::min<i64>(bs->nlp * 4, (i64)1 << 20));
        HIPCHK(h, hipHostMalloc((void **)&bs->h_tab, (size_t)cap * sizeof(IpmGatherSeg), hipHostMallocDefault));
        HIPCHK(h, hipMalloc((void **)&bs->d_tab, (size_t)cap * sizeof(IpmGatherSeg)));
        bs->tab_cap = cap;
    }
    if (need > bs->stage_cap) {
        if (bs->d_stage) { hipFree(bs->d_stage); bs->d_stage = nullptr; }
        bs->stage_cap = 0;
        HIPCHK(h, hipMalloc((void **)&bs->d_stage, (size_t)need * 8));
        bs->stage_cap = need;
    }
    i64 dst = 0, t = 0;
    for (i64 q = 0; q < nk; ++q)
        for (i64 w = 0; w < nwhat; ++w) {
            const std::vector<i64> &off = ipm_get_is_row(what[w]) ? bs->row_off : bs->col_off;
            const i64 k = lp[q], seg = off[(size_t)k + 1] - off[(size_t)k];
            bs->h_tab[t++] = IpmGatherSeg{src[what[w]] + off[(size_t)k], seg, dst};
            dst += seg;
        }
    HIPCHK(h, hipMemcpyAsync(bs->d_tab, bs->h_tab, (size_t)nseg * sizeof(IpmGatherSeg), hipMemcpyHostToDevice, h->stream));
    ipmb_launch_gather_segs(h->stream, bs->d_tab, nseg, maxlen, bs->d_stage);
    HIPCHK(h, hipMemcpyAsync(host, bs->d_stage, (size_t)need * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    return TLPK_OK;
}

}  // extern "C"
