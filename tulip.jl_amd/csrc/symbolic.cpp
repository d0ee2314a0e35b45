// symbolic.cpp -- host analyse phase: pattern of S = A*A', fill-reducing ordering, elimination
// tree, column counts, supernodes (fronts), relative indices, assembly lists for A*D*A' + Rd.
//
// Reference counterpart: the `cholesky(Symmetric(A*A' + I))` call in KKT.setup
// (/root/reference/src/KKT/Cholmod/spd.jl:14-17), i.e. CHOLMOD's analyse [ext].  The pattern of S
// is structural and constant over the IPM run (spd.jl:14,43), so everything computed here is
// reused by every update!/solve!.
#include "tlpk_host.hpp"
#include "schedule.hpp"
#include "../../include/tlpk.h"

#include <algorithm>
#include <atomic>
#include <thread>
#include <chrono>
#include <cstdio>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <mutex>
#include <functional>
#include <condition_variable>
#include <map>
#include <climits>

namespace tlpk {

// (the extend-add ranges of a parent front -- ea_cols, ea_npan, ea_nbounds, ea_bound -- are in schedule.hpp: the schedule builder cuts its tasks by them)
// Front assembly (k_front_assemble, FaTask) -- an experiment of round 4, OFF by default (TLPK_FA_MIN_F=512 turns it on): the panel of a front
// is FORMED tile by tile in LDS (S entries + children in child order, written once) instead of zero-fill + k_assemble + read-modify-write
// extend-add.  Its extend-add ranges are FA_CW = 16 columns wide, the same boundaries cut the rows of a tile.  Chosen per front in analyse_rank
// (Symbolic::front_fa): >= fa_min_f() rows and on average >= fa_density() contributions per entry of the front.
// Measured (profiles/r04_front_assembly.txt): on every large front (TLPK_FA_DENSITY=0) config C4 extend-add + assembly 6.9 -> 9.0 ms, north-star
// instance 12.4 -> 27.4 ms -- a tile sees ~100..400 children that each bring a few dozen entries, i.e. two dependent memory round trips per
// (child, tile) with nothing to overlap them, where the column-oriented k_extend_add streams whole child columns; on the linking (root) front only
// (one dense update matrix per diagonal block, the default density threshold): 7.16 vs 7.05 ms, no gain.  Parity-green (also on NaN-poisoned storage).
static inline i32 fa_min_f() {
    static const i32 v = [] { const char *e = std::getenv("TLPK_FA_MIN_F"); const int c = e ? std::atoi(e) : 0; return (i32)(c <= 0 ? INT32_MAX : c); }();
    return v;
}
static inline double fa_density() {
    static const double v = [] { const char *e = std::getenv("TLPK_FA_DENSITY"); return e ? std::atof(e) : 4.0; }();
    return v;
}

namespace {

// Liu's elimination-tree algorithm with path compression on a graph given in ORIGINAL labels
// plus a labelling iperm (old -> new); returns parent in NEW labels.
// Liu's algorithm with path compression for the nodes [i0, i1) of the ordering.  `parent` and `anc`
// (both initialised to -1 by the caller) are only touched at positions < i1 that are connected to
// the range, so disjoint ranges of mutually non-adjacent node sets can run concurrently.
static void etree_range(i32 i0, i32 i1, const std::vector<i64> &xadj, const std::vector<i32> &adj, const std::vector<i32> &perm,
                        const std::vector<i32> &iperm, std::vector<i32> &parent, std::vector<i32> &anc) {
    for (i32 i = i0; i < i1; ++i) {
        const i32 old = perm[i];
        for (i64 p = xadj[old]; p < xadj[old + 1]; ++p) {
            i32 k = iperm[adj[p]];
            while (k != -1 && k < i) {
                const i32 nxt = anc[k];
                anc[k] = i;
                if (nxt == -1) parent[k] = i;
                k = nxt;
            }
        }
    }
}
void etree_of(i32 m, const std::vector<i64> &xadj, const std::vector<i32> &adj, const std::vector<i32> &perm,
              const std::vector<i32> &iperm, std::vector<i32> &parent) {
    parent.assign(m, -1);
    std::vector<i32> anc(m, -1);
    etree_range(0, m, xadj, adj, perm, iperm, parent, anc);
}

// Postorder of a forest (children visited in increasing label order).  `skip[v]` nodes are cut
// out of the forest (their children become roots) and are not emitted.
void postorder_forest(i32 m, const std::vector<i32> &parent, const std::vector<char> *skip, std::vector<i32> &post) {
    std::vector<i32> head(m, -1), next(m, -1), roots;
    for (i32 v = m - 1; v >= 0; --v) {
        if (skip && (*skip)[v]) continue;
        const i32 p = parent[v];
        if (p == -1 || (skip && (*skip)[p])) continue;
        next[v] = head[p];
        head[p] = v;
    }
    post.clear();
    post.reserve(m);
    std::vector<i32> stack;
    for (i32 r = 0; r < m; ++r) {
        if (skip && (*skip)[r]) continue;
        const i32 p = parent[r];
        if (!(p == -1 || (skip && (*skip)[p]))) continue;
        stack.push_back(r);
        while (!stack.empty()) {
            const i32 v = stack.back();
            const i32 c = head[v];
            if (c != -1) { head[v] = next[c]; stack.push_back(c); }
            else { post.push_back(v); stack.pop_back(); }
        }
    }
}

}  // namespace

static int fail(Symbolic &S, int code, const std::string &msg) { S.error = msg; return code; }

// Host threads for the embarrassingly parallel parts of the analyse phase.  fn(thread, i) is called once
// for every i in [0, n), items handed out dynamically; the result never depends on the number of
// threads (every item writes its own outputs).  Returns false if a worker threw (out of memory).
// Sharded runs (round-5 review): every one of N ranks -- N processes of a multi-GPU launch, or the N per-shard threads of tlpk_create_multi -- runs this
// analysis at the same time on the same host: the default thread count is divided by N (8 ranks would otherwise start 512 analyse threads on a host that
// grants the job 16 - 256 CPUs).  Set at the top of analyse_common / analyse_rank from Options.nranks; an explicit TLPK_HOST_THREADS is taken as given.
static thread_local i64 g_host_thread_div = 1;
static unsigned host_threads(i64 n) {
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    // up to a quarter of the hardware threads, at most 64 (env TLPK_HOST_THREADS overrides): the per-front / per-block phases
    // of a block-angular LP with 64 diagonal blocks were 3-4 rounds deep with the old cap of 16 on a 256-thread host.  NOT capped by the
    // container's CPU quota (16 CPUs on the GPU boxes): the phases are bursts of well under the 100-ms accounting period, 64 threads are the
    // fastest setting there (C4 281 ms against 347 with 16; north-star LP 1093 against 1258: tools/analyse_threads_probe.py) -- unlike the
    // seconds-long OpenMP teams of the CPU comparator, which the quota throttles
    static const i64 cap = [] { const char *e = std::getenv("TLPK_HOST_THREADS"); return e ? std::max<i64>(1, std::atoll(e)) : (i64)64; }();
    const i64 mine = std::getenv("TLPK_HOST_THREADS") ? cap : std::max<i64>(1, std::min<i64>(cap, std::max<i64>(16, hw / 4)) / g_host_thread_div);
    return (unsigned)std::max<i64>(1, std::min<i64>({(i64)hw, mine, n}));
}
// Round 6: the worker threads of ONE analyse call.  parallel_for used to create and join its threads on every call -- ~50 calls per analyse (two per level of the
// supernodal tree alone) x up to 63 threads: tens of milliseconds of clone / join on a 250-ms analyse.  An AnalysePool lives for the duration of an analyse_common /
// analyse_rank call (scope object: nothing survives the call, nothing to make fork-safe), its threads are created on first use and sleep on a condition variable
// between jobs.  A job = (worker function, number of participants); thread t of the pool runs worker(t + 1), the caller runs worker(0) and waits for the rest.
// Nested parallel_for calls (none today) and calls outside an analyse fall back to the create-and-join form.
struct AnalysePool {
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv, cv_done;
    const std::function<void(unsigned)> *job = nullptr;
    unsigned want = 0, done = 0;
    unsigned long long gen = 0;
    bool stop = false, busy = false;
    ~AnalysePool() {
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv.notify_all();
        for (auto &t : th) t.join();
    }
    void loop(unsigned idx) {
        unsigned long long seen = 0;
        for (;;) {
            const std::function<void(unsigned)> *j = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || gen != seen; });
                if (stop) return;
                seen = gen;
                if (idx < want) j = job;
            }
            if (j) {
                (*j)(idx + 1);
                std::lock_guard<std::mutex> lk(mu);
                if (++done == want) cv_done.notify_one();
            }
        }
    }
    // runs worker(0 .. nthreads - 1); false = the pool cannot serve (busy: a nested call) and the caller must use its own threads
    bool run(unsigned nthreads, const std::function<void(unsigned)> &worker) {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (busy) return false;
            busy = true;
        }
        unsigned helpers = nthreads - 1;
        try { while (th.size() < helpers) { const unsigned idx = (unsigned)th.size(); th.emplace_back([this, idx] { loop(idx); }); } }
        catch (...) { helpers = (unsigned)th.size(); }      // thread / pid limits of a container: go on with the threads we have (the workers drain the items whoever runs them)
        {
            std::lock_guard<std::mutex> lk(mu);
            job = &worker; want = helpers; done = 0; ++gen;
        }
        cv.notify_all();
        worker(0);
        {
            std::unique_lock<std::mutex> lk(mu);
            cv_done.wait(lk, [&] { return done == want; });
            job = nullptr; want = 0; busy = false;
        }
        return true;
    }
};
static thread_local AnalysePool *g_analyse_pool = nullptr;      // the pool of the analyse running on this thread (TLPK_ANALYSE_POOL=0: none)
struct AnalysePoolScope {
    AnalysePool pool; AnalysePool *prev;
    AnalysePoolScope() : prev(g_analyse_pool) {
        static const bool on = [] { const char *e = std::getenv("TLPK_ANALYSE_POOL"); return !e || std::atoi(e) != 0; }();
        if (on && !prev) g_analyse_pool = &pool;
    }
    ~AnalysePoolScope() { g_analyse_pool = prev; }
};

// `chunk` consecutive items go to the same thread (neighbouring items usually write neighbouring memory:
// item-by-item hand-out made the threads fight over cache lines on instances with 400 000 small fronts).
template <class F>
static bool parallel_for(i64 n, unsigned nthreads, F &&fn, i64 chunk = 1) {
    std::atomic<i64> next{0};
    std::atomic<int> failed{0};
    auto worker = [&](unsigned tid) {
        try {
            for (i64 i0; (i0 = next.fetch_add(chunk)) < n;)
                for (i64 i = i0; i < std::min(n, i0 + chunk); ++i) fn(tid, i);
        } catch (...) { failed = 1; }
    };
    if (nthreads <= 1) { worker(0); return !failed; }
    if (g_analyse_pool) {
        const std::function<void(unsigned)> w = worker;
        if (g_analyse_pool->run(nthreads, w)) return !failed;
    }
    // A thread that cannot be created (thread / pid limits of a container) is not an error: the
    // threads that did start and the calling thread drain the work.  Nothing may escape while a
    // started thread is still joinable (the vector's destructor would call std::terminate).
    std::vector<std::thread> pool;
    try {
        pool.reserve(nthreads);
        for (unsigned t = 1; t < nthreads; ++t) pool.emplace_back(worker, t);
    } catch (...) { /* std::system_error / bad_alloc: go on with the threads we have */ }
    worker(0);
    for (auto &th : pool) th.join();
    return !failed;
}

// Same, for call sites without an error path of their own: a failed worker (out of memory) becomes a
// std::bad_alloc AFTER every thread has been joined; tlpk_create maps it to TLPK_OOM.
template <class F>
static void parallel_for_throw(i64 n, unsigned nthreads, F &&fn, i64 chunk = 1) {
    if (!parallel_for(n, nthreads, std::forward<F>(fn), chunk)) throw std::bad_alloc();
}

// independent iterations over [0, n) in chunks of 64 K on the host threads (the element-wise relabelling loops of the analyse: 2e6 scattered 4-byte accesses each on
// the north-star LP, 5 - 10 ms apiece on one thread)
template <class F>
static void par_chunks(i64 n, F &&fn) {
    constexpr i64 CH = 65536;
    const i64 nch = (n + CH - 1) / CH;
    if (nch <= 1) { if (n > 0) fn((i64)0, n); return; }
    parallel_for_throw(nch, host_threads(nch), [&](unsigned, i64 ch) { fn(ch * CH, std::min(n, (ch + 1) * CH)); });
}

// The analyse phase in two parts.  analyse_common: everything that does not depend on the rank of a sharded run -- copy of
// A, the graph of A*A', the ordering, the elimination tree, column counts, supernodes, amalgamation, front structures (87 % of
// the time on config C4).  analyse_rank: ownership, storage offsets, relative indices, gather / assembly lists and the launch
// schedules of ONE rank.  tlpk_create runs both; tlpk_create_multi runs the common part once and the rank part per device.
int analyse_common(Symbolic &S, i64 m64, i64 n64, const i64 *colptr, const i64 *rowval, const double *nzval,
                   int base, const Options &opt) {
    PhaseTimer pt;
    AnalysePoolScope pool_scope;
    g_host_thread_div = opt.analyse_div > 0 ? opt.analyse_div : std::max<i32>(1, opt.nranks);
    if (m64 < 0 || n64 < 0 || (base != 0 && base != 1) || !colptr) return fail(S, TLPK_BADARG, "bad dimensions or index base");
    if (m64 >= (i64)1 << 31 || n64 >= (i64)1 << 31) return fail(S, TLPK_TOO_LARGE, "m or n exceeds int32");
    const i64 nnz = colptr[n64] - base;
    if (nnz < 0 || nnz >= (i64)1 << 31) return fail(S, TLPK_TOO_LARGE, "nnz(A) exceeds int32");
    if (nnz > 0 && (!rowval || !nzval)) return fail(S, TLPK_BADARG, "null rowval/nzval");
    const i32 m = (i32)m64, n = (i32)n64;
    S.m = m; S.n = n; S.nnzA = nnz;
    if (opt.nranks < 1 || opt.rank < 0 || opt.rank >= opt.nranks) return fail(S, TLPK_BADARG, "bad rank/nranks");
    if (opt.nranks > 1 && !opt.row_block) return fail(S, TLPK_BADARG, "sharding needs row_block (general sparse LPs are single-GPU)");

    pt.mark("copy A / CSR");
    // ---- 1. copy A (CSC) and build CSR ----
    S.Ap.resize((size_t)n + 1); S.Ai.resize((size_t)nnz); S.Ax.resize((size_t)nnz); S.Acol.resize((size_t)nnz);
    for (i32 j = 0; j <= n; ++j) {
        S.Ap[j] = colptr[j] - base;
        if (S.Ap[j] < 0 || S.Ap[j] > nnz || (j > 0 && S.Ap[j] < S.Ap[j - 1])) return fail(S, TLPK_BADARG, "colptr not monotone");
    }
    // (round 5: on the host threads.  The copy by chunks of columns; the transposition by ranges of ROWS: every thread scans the row indices of the whole matrix -- a
    // sequential read of 4 nnz bytes -- and places the entries of its own rows, in column order: the same CSR arrays as the serial loop, without a shared cursor.)
    {
        constexpr i64 CH = 8192;
        const i64 nch = ((i64)n + CH - 1) / CH;
        std::atomic<int> bad{0};
        if (!parallel_for(nch, host_threads(nch), [&](unsigned, i64 ch) {
                const i32 j1 = (i32)std::min<i64>(n, (ch + 1) * CH);
                for (i32 j = (i32)(ch * CH); j < j1; ++j)
                    for (i64 p = S.Ap[j]; p < S.Ap[j + 1]; ++p) {
                        const i64 r = rowval[p] - base;
                        if (r < 0 || r >= m) { bad = 1; continue; }
                        S.Ai[p] = (i32)r; S.Ax[p] = nzval[p]; S.Acol[p] = j;
                    }
            })) return fail(S, TLPK_OOM, "out of memory in the analyse phase");
        if (bad) return fail(S, TLPK_BADARG, "row index out of range");
    }
    S.Tp.assign((size_t)m + 1, 0);
    S.Tj.resize((size_t)nnz); S.Tpos.resize((size_t)nnz);
    {
        const unsigned nt = host_threads(std::max<i64>(1, nnz / 200000));          // row ranges, one per thread
        const i64 rstep = ((i64)m + nt - 1) / nt;
        if (!parallel_for(nt, nt, [&](unsigned, i64 t) {                             // counts of the thread's rows
                const i64 r0 = t * rstep, r1 = std::min<i64>(m, r0 + rstep);
                if (r0 >= r1) return;
                for (i64 p = 0; p < nnz; ++p) { const i64 r = S.Ai[p]; if (r >= r0 && r < r1) S.Tp[r + 1]++; }
            })) return fail(S, TLPK_OOM, "out of memory in the analyse phase");
        for (i32 i = 0; i < m; ++i) S.Tp[i + 1] += S.Tp[i];
        if (!parallel_for(nt, nt, [&](unsigned, i64 t) {
                const i64 r0 = t * rstep, r1 = std::min<i64>(m, r0 + rstep);
                if (r0 >= r1) return;
                std::vector<i64> cur(S.Tp.begin() + r0, S.Tp.begin() + r1);
                for (i64 p = 0; p < nnz; ++p) {
                    const i64 r = S.Ai[p];
                    if (r < r0 || r >= r1) continue;
                    const i64 q = cur[(size_t)(r - r0)]++;
                    S.Tj[q] = S.Acol[p]; S.Tpos[q] = (i32)p;
                }
            })) return fail(S, TLPK_OOM, "out of memory in the analyse phase");
    }

    pt.mark("block structure");
    // ---- 2. block-angular structure (optional) ----
    std::vector<i32> &row_block = S.row_block_v, &col_block = S.col_block_v;
    row_block.clear(); col_block.clear();
    i32 nblocks = 0, nlink = 0;
    if (opt.row_block) {
        row_block.resize(m);
        for (i32 i = 0; i < m; ++i) {
            const i64 b = opt.row_block[i];
            if (b < -1 || b >= (i64)1 << 30) return fail(S, TLPK_BADARG, "row_block out of range");
            row_block[i] = (i32)b;
            if (b >= 0) nblocks = std::max(nblocks, (i32)b + 1); else ++nlink;
        }
        col_block.assign(n, -1);
        for (i32 j = 0; j < n; ++j)
            for (i64 p = S.Ap[j]; p < S.Ap[j + 1]; ++p) {
                const i32 b = row_block[S.Ai[p]];
                if (b < 0) continue;
                if (col_block[j] == -1) col_block[j] = b;
                else if (col_block[j] != b) return fail(S, TLPK_BADARG, "row_block is not block-angular: a column spans two blocks");
            }
    }
    S.nblocks = nblocks;

    pt.mark("graph of AA'");
    // ---- 3. adjacency graph of A*A' (original labels, no diagonal, both directions) ----
    std::vector<i64> xadj((size_t)m + 1, 0);
    std::vector<i32> adj;
    {
        // rows are independent: chunks of rows on the host threads, count then fill (the marker array of a
        // thread is stamped with 2k / 2k+1, so the two passes and the rows of a chunk never collide)
        constexpr i64 CH = 4096;
        const i64 nch = ((i64)m + CH - 1) / CH;
        const unsigned nthreads = host_threads(nch);
        std::vector<std::vector<i64>> t_mark(nthreads);
        auto sweep = [&](bool fill) {
            return parallel_for(nch, nthreads, [&](unsigned tid, i64 ch) {
                std::vector<i64> &mark = t_mark[tid];
                if (mark.empty()) mark.assign(m, -1);
                for (i32 k = (i32)(ch * CH); k < (i32)std::min<i64>(m, (ch + 1) * CH); ++k) {
                    const i64 stamp = 2 * (i64)k + (fill ? 1 : 0);
                    mark[k] = stamp;
                    i64 c = fill ? xadj[k] : 0;
                    for (i64 q = S.Tp[k]; q < S.Tp[k + 1]; ++q) {
                        const i32 j = S.Tj[q];
                        for (i64 p = S.Ap[j]; p < S.Ap[j + 1]; ++p) {
                            const i32 i = S.Ai[p];
                            if (mark[i] != stamp) { mark[i] = stamp; if (fill) adj[c] = i; ++c; }
                        }
                    }
                    if (!fill) xadj[k + 1] = c;
                }
            });
        };
        if (!sweep(false)) return fail(S, TLPK_OOM, "out of memory while building the graph of A*A'");
        for (i32 k = 0; k < m; ++k) xadj[k + 1] += xadj[k];
        adj.resize((size_t)xadj[m]);
        if (!sweep(true)) return fail(S, TLPK_OOM, "out of memory while building the graph of A*A'");
    }

    pt.mark("ordering (AMD)");
    // ---- 4. fill-reducing ordering ----
    std::vector<i32> order0;
    order0.reserve(m);
    std::vector<char> is_link(m, 0);
    // dense-column nodes (analyse_dense, general path): the constraint nodes [0, mc) are ordered as the K1 matrix of A_s alone -- the subgraph
    // without the dense nodes --, the dense nodes follow as the forced root front (is_link)
    const i32 mc = m - (i32)opt.n_dense;
    auto append_dense = [&]() { for (i32 v = mc; v < m; ++v) { order0.push_back(v); is_link[v] = 1; ++nlink; } };
    if (opt.ordering == TLPK_ORDER_USER) {
        if (!opt.user_perm) return fail(S, TLPK_BADARG, "user_perm is null");
        std::vector<char> seen(mc, 0);
        for (i32 i = 0; i < mc; ++i) {
            const i64 v = opt.user_perm[i];
            if (v < 0 || v >= mc || seen[v]) return fail(S, TLPK_BADARG, "user_perm is not a permutation");
            seen[v] = 1; order0.push_back((i32)v);
        }
        if (opt.row_block) return fail(S, TLPK_BADARG, "user_perm cannot be combined with row_block");
        append_dense();
    } else if (!opt.row_block) {
        if (opt.ordering == TLPK_ORDER_NATURAL) { order0.resize(mc); std::iota(order0.begin(), order0.end(), 0); }
        else if (mc == m) amd_order(m, xadj, adj, order0);
        else {
            std::vector<i64> cx((size_t)mc + 1, 0);
            std::vector<i32> ca;
            ca.reserve((size_t)xadj[mc]);
            for (i32 v = 0; v < mc; ++v) {
                for (i64 p = xadj[v]; p < xadj[v + 1]; ++p) if (adj[p] < mc) ca.push_back(adj[p]);
                cx[(size_t)v + 1] = (i64)ca.size();
            }
            amd_order(mc, cx, ca, order0);
        }
        append_dense();
    } else {
        // each diagonal block on its own (blocks are mutually non-adjacent in S); linking rows last
        std::vector<std::vector<i32>> members(nblocks);
        for (i32 i = 0; i < m; ++i) if (row_block[i] >= 0) members[row_block[i]].push_back(i);
        std::vector<i32> local(m, -1);
        for (i32 b = 0; b < nblocks; ++b) for (size_t t = 0; t < members[b].size(); ++t) local[members[b][t]] = (i32)t;
        // the blocks are independent graphs: ordered concurrently on the host's cores (the result does
        // not depend on the number of threads: every block is ordered by itself)
        std::vector<std::vector<i32>> border(nblocks);
        auto order_block = [&](i32 b) {
            const auto &mb = members[b];
            const i32 nb = (i32)mb.size();
            if (opt.ordering == TLPK_ORDER_NATURAL) { border[b].resize(nb); std::iota(border[b].begin(), border[b].end(), 0); return; }
            std::vector<i64> bx((size_t)nb + 1, 0);
            std::vector<i32> ba;
            for (i32 t = 0; t < nb; ++t) {
                const i32 v = mb[t];
                for (i64 p = xadj[v]; p < xadj[v + 1]; ++p) {
                    const i32 u = adj[p];
                    if (row_block[u] == b) ba.push_back(local[u]);
                }
                bx[t + 1] = (i64)ba.size();
            }
            amd_order(nb, bx, ba, border[b]);
        };
        {
            const unsigned nthreads = host_threads(nblocks);
            if (std::getenv("TLPK_TIMING")) std::fprintf(stderr, "[tlpk analyse] ordering %d blocks on %u threads\n", (int)nblocks, nthreads);
            if (!parallel_for(nblocks, nthreads, [&](unsigned, i64 b) { order_block((i32)b); }))
                return fail(S, TLPK_OOM, "out of memory while ordering the diagonal blocks");
        }
        for (i32 b = 0; b < nblocks; ++b) for (i32 t : border[b]) order0.push_back(members[b][t]);
        for (i32 i = 0; i < m; ++i) if (row_block[i] < 0) { order0.push_back(i); is_link[i] = 1; }
    }
    if ((i32)order0.size() != m) return fail(S, TLPK_INTERNAL, "ordering did not return a permutation");

    pt.mark("etree");
    // ---- 5. elimination tree, postorder ----
    std::vector<i32> iperm0(m);
    par_chunks(m, [&](i64 lo, i64 hi) { for (i64 i = lo; i < hi; ++i) iperm0[order0[i]] = (i32)i; });
    std::vector<i32> parent0;
    if (opt.row_block && nblocks >= 2 && opt.ordering != TLPK_ORDER_USER) {
        // block-angular: the ordering lists block after block, then the linking rows.  The nodes of a block
        // are adjacent only to their own block and to linking rows (which come later and are skipped by
        // the k < i test), so the blocks' ranges are independent; the linking rows follow sequentially.
        std::vector<i32> bstart;
        for (i32 i = 0; i < m; ++i)
            if (!is_link[order0[i]] && (i == 0 || row_block[order0[i]] != row_block[order0[i - 1]])) bstart.push_back(i);
        const i32 first_link0 = m - nlink;
        bstart.push_back(first_link0);
        parent0.assign(m, -1);
        std::vector<i32> anc(m, -1);
        const i64 nb = (i64)bstart.size() - 1;
        parallel_for_throw(nb, host_threads(nb), [&](unsigned, i64 b) { etree_range(bstart[b], bstart[b + 1], xadj, adj, order0, iperm0, parent0, anc); });
        etree_range(first_link0, m, xadj, adj, order0, iperm0, parent0, anc);
    } else
        etree_of(m, xadj, adj, order0, iperm0, parent0);
    // final order: postorder of the forest without the linking nodes, then the linking nodes
    std::vector<char> skip(m, 0);
    par_chunks(m, [&](i64 lo, i64 hi) { for (i64 i = lo; i < hi; ++i) skip[i] = is_link[order0[i]]; });
    std::vector<i32> post0;
    postorder_forest(m, parent0, nlink ? &skip : nullptr, post0);
    for (i32 i = 0; i < m; ++i) if (skip[i]) post0.push_back(i);
    if ((i32)post0.size() != m) return fail(S, TLPK_INTERNAL, "postorder lost nodes");
    S.perm.resize(m); S.iperm.resize(m);
    std::vector<i32> relabel(m);               // order0-label -> final label
    par_chunks(m, [&](i64 lo, i64 hi) { for (i64 k = lo; k < hi; ++k) { S.perm[k] = order0[post0[k]]; relabel[post0[k]] = (i32)k; } });
    par_chunks(m, [&](i64 lo, i64 hi) { for (i64 k = lo; k < hi; ++k) S.iperm[S.perm[k]] = (i32)k; });
    S.parent.assign(m, -1);
    par_chunks(m, [&](i64 lo, i64 hi) { for (i64 v = lo; v < hi; ++v) if (parent0[v] != -1) S.parent[relabel[v]] = relabel[parent0[v]]; });
    {
        std::atomic<int> bad_topo{0};
        par_chunks(m, [&](i64 lo, i64 hi) { for (i64 k = lo; k < hi; ++k) if (S.parent[k] != -1 && S.parent[k] <= k) bad_topo = 1; });
        if (bad_topo) return fail(S, TLPK_INTERNAL, "etree not topological");
    }
    const i32 first_link = m - nlink;

    pt.mark("pattern of S");
    // ---- 6. permuted lower pattern of S (rebuilt if the amalgamation re-orders columns) ----
    auto build_pattern = [&]() {
        // columns are independent: chunks of columns on the host threads
        constexpr i64 CH = 2048;
        const i64 nch = ((i64)m + CH - 1) / CH;
        const unsigned nthreads = host_threads(nch);
        S.Sp.assign((size_t)m + 1, 0);
        parallel_for_throw(nch, nthreads, [&](unsigned, i64 ch) {
            for (i32 kk = (i32)(ch * CH); kk < (i32)std::min<i64>(m, (ch + 1) * CH); ++kk) {
                const i32 k = S.perm[kk];
                i64 c = 1;
                for (i64 p = xadj[k]; p < xadj[k + 1]; ++p) if (S.iperm[adj[p]] > kk) ++c;
                S.Sp[kk + 1] = c;
            }
        });
        for (i32 kk = 0; kk < m; ++kk) S.Sp[kk + 1] += S.Sp[kk];
        S.nnzS = S.Sp[m];
        S.Si.resize((size_t)S.nnzS);
        parallel_for_throw(nch, nthreads, [&](unsigned, i64 ch) {
            for (i32 kk = (i32)(ch * CH); kk < (i32)std::min<i64>(m, (ch + 1) * CH); ++kk) {
                const i32 k = S.perm[kk];
                i64 q = S.Sp[kk];
                S.Si[q++] = kk;
                for (i64 p = xadj[k]; p < xadj[k + 1]; ++p) { const i32 ii = S.iperm[adj[p]]; if (ii > kk) S.Si[q++] = ii; }
                std::sort(S.Si.begin() + S.Sp[kk] + 1, S.Si.begin() + q);
            }
        });
    };
    build_pattern();

    pt.mark("column counts");
    // ---- 7. column counts (Gilbert, Ng & Peyton 1994: row-subtree leaves + LCA by union-find) ----
    {
        std::vector<i32> tpost;
        postorder_forest(m, S.parent, nullptr, tpost);        // a true postorder of the final tree
        std::vector<i32> pidx(m), first(m), delta(m, 0), maxfirst(m, -1), prevleaf(m, -1), anc(m);
        for (i32 k = 0; k < m; ++k) pidx[tpost[k]] = k;
        for (i32 v = 0; v < m; ++v) { first[v] = pidx[v]; anc[v] = v; }
        for (i32 k = 0; k < m; ++k) {                          // first descendant, children before parents
            const i32 v = tpost[k], p = S.parent[v];
            if (p != -1) first[p] = std::min(first[p], first[v]);
        }
        for (i32 k = 0; k < m; ++k) {
            const i32 j = tpost[k];
            delta[j] += (first[j] == k) ? 1 : 0;               // j is a leaf of the etree
            if (S.parent[j] != -1) delta[S.parent[j]]--;
            for (i64 p = S.Sp[j] + 1; p < S.Sp[j + 1]; ++p) {
                const i32 i = S.Si[p];                         // i is an ancestor of j, S[i,j] != 0
                if (first[j] <= maxfirst[i]) continue;         // j is not a leaf of row subtree T^i
                maxfirst[i] = first[j];
                const i32 jprev = prevleaf[i];
                prevleaf[i] = j;
                delta[j]++;
                if (jprev != -1) {
                    i32 q = jprev;
                    while (anc[q] != q) q = anc[q];
                    for (i32 s = jprev; s != q;) { const i32 t = anc[s]; anc[s] = q; s = t; }
                    delta[q]--;
                }
            }
            if (S.parent[j] != -1) anc[j] = S.parent[j];
        }
        S.colcount.assign(m, 0);
        for (i32 k = 0; k < m; ++k) {
            const i32 j = tpost[k];
            S.colcount[j] += delta[j];
            if (S.parent[j] != -1) S.colcount[S.parent[j]] += S.colcount[j];
        }
    }
    S.nnzL = 0; S.flops_chol = 0;
    for (i32 j = 0; j < m; ++j) {
        if (S.colcount[j] < 1) return fail(S, TLPK_INTERNAL, "column count < 1");
        S.nnzL += S.colcount[j]; S.flops_chol += (double)S.colcount[j] * (double)S.colcount[j];
    }

    pt.mark("fundamental supernodes");
    // ---- 8. fundamental supernodes ----
    // start[s] = first column.  j joins j-1 when parent[j-1] == j and the structures nest exactly
    // (count[j-1] == count[j] + 1).  Linking columns form one forced root front.
    std::vector<i32> sn_start;
    for (i32 j = 0; j < m; ++j) {
        bool join = false;
        if (j > 0) {
            if (j > first_link) join = true;                                 // inside the forced root
            else if (j == first_link) join = false;
            else join = (S.parent[j - 1] == j && S.colcount[j - 1] == S.colcount[j] + 1);
        }
        if (!join) sn_start.push_back(j);
    }
    sn_start.push_back(m);
    i32 ns_total = 0;
    std::vector<i32> &sparent = S.sparent_v;

    pt.mark("fronts");
    // ---- 9. supernodal tree and front row structures (for a given column partition) ----
    // rows == false: only the supernodal tree and the front sizes (exact for fundamental supernodes:
    // f = column count of the first column) -- all the amalgamation looks at; the row structures are
    // then built once, for the final partition
    auto build_fronts = [&](bool rows) -> int {
        ns_total = (i32)sn_start.size() - 1;
        S.nsuper = ns_total;
        S.sn_of_col.resize(m);
        par_chunks(ns_total, [&](i64 lo, i64 hi) { for (i64 s = lo; s < hi; ++s) for (i32 j = sn_start[s]; j < sn_start[s + 1]; ++j) S.sn_of_col[j] = (i32)s; });
        S.fronts.assign(ns_total, FrontDesc{});
        sparent.assign(ns_total, -1);
        for (i32 s = 0; s < ns_total; ++s) {
            // parent front: the one holding the etree parent of the supernode's last column
            const i32 pc = S.parent[sn_start[s + 1] - 1];
            sparent[s] = (pc == -1) ? -1 : S.sn_of_col[pc];
            if (sparent[s] != -1 && sparent[s] <= s) return fail(S, TLPK_INTERNAL, "supernodal tree not topological");
        }
        std::vector<i32> nchild(ns_total, 0);
        for (i32 s = 0; s < ns_total; ++s) if (sparent[s] != -1) nchild[sparent[s]]++;
        i32 acc = 0;
        for (i32 s = 0; s < ns_total; ++s) { S.fronts[s].child_ptr = acc; S.fronts[s].nchild = 0; acc += nchild[s]; }
        S.children.assign(acc, -1);
        for (i32 s = 0; s < ns_total; ++s) if (sparent[s] != -1) {
            FrontDesc &p = S.fronts[sparent[s]];
            S.children[p.child_ptr + p.nchild++] = s;
        }
        // rows(s) = cols(s) ++ sorted union of the below-diagonal structure of every column of s
        // and of the children's rows; merged (relaxed) supernodes carry explicit zeros.
        if (!rows) {
            for (i32 s = 0; s < ns_total; ++s) {
                FrontDesc &w = S.fronts[s];
                const i32 j0 = sn_start[s];
                w.ns = sn_start[s + 1] - j0; w.f = (i32)S.colcount[j0]; w.col0 = j0; w.parent = sparent[s];
            }
            return TLPK_OK;
        }
        // A front needs the below-rows of its children: level by level, deepest first, the fronts of a
        // level on the host threads (each with its own marker array), then one sequential pass lays the
        // lists out in front order.
        std::vector<std::vector<i32>> below(ns_total);
        {
            std::vector<i32> sdepth(ns_total, 0);
            i32 maxd = 0;
            for (i32 s = ns_total - 1; s >= 0; --s) { sdepth[s] = (sparent[s] == -1) ? 0 : sdepth[sparent[s]] + 1; maxd = std::max(maxd, sdepth[s]); }
            std::vector<std::vector<i32>> bylevel(maxd + 1);
            for (i32 s = 0; s < ns_total; ++s) bylevel[sdepth[s]].push_back(s);
            const unsigned nthreads = host_threads(ns_total);
            std::vector<std::vector<i32>> t_mark(nthreads);
            for (i32 d = maxd; d >= 0; --d) {
                const std::vector<i32> &lv = bylevel[d];
                const bool ok = parallel_for((i64)lv.size(), std::min<unsigned>(nthreads, (unsigned)std::max<size_t>(1, lv.size())), [&](unsigned tid, i64 q) {
                    const i32 s = lv[q];
                    std::vector<i32> &mark = t_mark[tid];
                    if (mark.empty()) mark.assign(m, -1);
                    const i32 j0 = sn_start[s], j1 = sn_start[s + 1] - 1;
                    std::vector<i32> &tmp = below[s];
                    for (i32 j = j0; j <= j1; ++j)
                        for (i64 p = S.Sp[j] + 1; p < S.Sp[j + 1]; ++p) {
                            const i32 i = S.Si[p];
                            if (i > j1 && mark[i] != s) { mark[i] = s; tmp.push_back(i); }
                        }
                    const FrontDesc &fd = S.fronts[s];
                    for (i32 t = 0; t < fd.nchild; ++t)
                        for (const i32 i : below[S.children[fd.child_ptr + t]])
                            if (i > j1 && mark[i] != s) { mark[i] = s; tmp.push_back(i); }
                    std::sort(tmp.begin(), tmp.end());
                }, 16);
                if (!ok) return fail(S, TLPK_OOM, "out of memory while building the front structures");
            }
        }
        S.rowidx.clear();
        {
            size_t total = (size_t)m;
            for (i32 s = 0; s < ns_total; ++s) total += below[s].size();
            S.rowidx.reserve(total);
        }
        S.max_front = 0;
        for (i32 s = 0; s < ns_total; ++s) {
            const i32 j0 = sn_start[s], j1 = sn_start[s + 1] - 1;
            const std::vector<i32> &tmp = below[s];
            FrontDesc &w = S.fronts[s];
            w.rowoff = (i64)S.rowidx.size();
            w.ns = j1 - j0 + 1;
            w.f = w.ns + (i32)tmp.size();
            w.col0 = j0;
            w.parent = sparent[s];
            for (i32 j = j0; j <= j1; ++j) S.rowidx.push_back(j);
            S.rowidx.insert(S.rowidx.end(), tmp.begin(), tmp.end());
            if (w.f < S.colcount[j0]) return fail(S, TLPK_INTERNAL, "front smaller than its first column count");
            if (!tmp.empty() && sparent[s] == -1) return fail(S, TLPK_INTERNAL, "root front with rows below");
            if (!tmp.empty() && S.sn_of_col[tmp[0]] != sparent[s]) return fail(S, TLPK_INTERNAL, "first below-row is not in the parent front");
            S.max_front = std::max<i64>(S.max_front, w.f);
        }
        return TLPK_OK;
    };
    const bool will_relax = opt.relax && (i32)sn_start.size() - 1 > 1;
    { const int rc = build_fronts(!will_relax); if (rc != TLPK_OK) return rc; }

    pt.mark("amalgamation");
    // ---- 9b. relaxed amalgamation (any child, not only the adjacent one) ----
    // A child front c is merged into its parent p when either the explicit zeros stay small
    // (CHOLMOD-style width classes) or -- the multifrontal criterion -- padding c's ns_c columns
    // to the parent's rows costs fewer flops than shipping its rs_c x rs_c update matrix through
    // HBM would cost in time (extra_flops < GAMMA * rs_c^2, GAMMA ~ flop rate x bytes per entry /
    // bandwidth) without growing memory.  Merged members become contiguous by re-ordering the
    // columns with another topological order of the same elimination tree (identical fill).
    if (opt.relax && ns_total > 1) {
        double GAMMA = 25.0;
        if (const char *e = std::getenv("TLPK_RELAX_GAMMA")) GAMMA = std::atof(e);    // tuning knob
        double GAMMA_TALL = 400.0, TALL_RATIO = 0.5;                                  // (read once: two getenv calls per candidate were a fifth of this phase)
        if (const char *e = std::getenv("TLPK_RELAX_GAMMA_TALL")) GAMMA_TALL = std::atof(e);
        if (const char *e = std::getenv("TLPK_RELAX_TALL_RATIO")) TALL_RATIO = std::atof(e);
        const i32 forced_root = nlink ? ns_total - 1 : -1;
        std::vector<i32> into(ns_total, -1);
        std::vector<double> cns(ns_total), cf(ns_total), cz(ns_total, 0.0);
        // children lists as flat arrays (400 000 fronts on the north-star LP: a vector per front was a third of this phase): the initial lists in
        // `kid0` (children in ascending order), the list a processed front KEEPS appended to `kept`; kid_list(x) = whichever is current
        std::vector<i32> kid0_ptr((size_t)ns_total + 1, 0), kid0((size_t)ns_total), kept, kept_ptr((size_t)ns_total, -1), kept_cnt((size_t)ns_total, 0);
        for (i32 s = 0; s < ns_total; ++s) {
            cns[s] = S.fronts[s].ns; cf[s] = S.fronts[s].f;
            if (sparent[s] != -1) kid0_ptr[(size_t)sparent[s] + 1]++;
        }
        for (i32 s = 0; s < ns_total; ++s) kid0_ptr[(size_t)s + 1] += kid0_ptr[(size_t)s];
        {
            std::vector<i32> fill(kid0_ptr.begin(), kid0_ptr.end() - 1);
            for (i32 s = 0; s < ns_total; ++s) if (sparent[s] != -1) kid0[(size_t)fill[(size_t)sparent[s]]++] = s;
        }
        kept.reserve((size_t)ns_total);
        auto kid_list = [&](i32 x, const i32 *&first, i32 &count) {
            if (kept_ptr[(size_t)x] >= 0) { first = kept.data() + kept_ptr[(size_t)x]; count = kept_cnt[(size_t)x]; }
            else { first = kid0.data() + kid0_ptr[(size_t)x]; count = kid0_ptr[(size_t)x + 1] - kid0_ptr[(size_t)x]; }
        };
        std::vector<i32> cand, keep;
        bool any_merge = false;
        for (i32 p = 0; p < ns_total; ++p) {
            if (p == forced_root || kid0_ptr[(size_t)p + 1] == kid0_ptr[(size_t)p]) continue;
            cand.assign(kid0.begin() + kid0_ptr[(size_t)p], kid0.begin() + kid0_ptr[(size_t)p + 1]); keep.clear();
            std::sort(cand.begin(), cand.end(), [&](i32 a, i32 b) { return (cf[a] - cns[a]) > (cf[b] - cns[b]); });
            for (size_t idx = 0; idx < cand.size(); ++idx) {
                const i32 c = cand[idx];
                const double nc = cns[c], fc = cf[c], np = cns[p], fp = cf[p];
                const double rsc = fc - nc, fnew = nc + fp;
                const double extra_zeros = nc * (fnew - fc);
                const double newz = cz[c] + cz[p] + extra_zeros;
                const double total = (nc + np) * fnew;
                const double width = nc + np;
                const double extra_flops = nc * (fnew * fnew - fc * fc);
                // the zero-fraction classes bound MEMORY; the last, unbounded-width class also needs a bound on the padded FLOPS
                // (a 5-row leaf column absorbed by a 4 500-row front costs 2e7 flops of zeros for 25 flops of work)
                static const double ZFRAC = [] { const char *e = std::getenv("TLPK_RELAX_ZFRAC"); return e ? std::atof(e) : 0.05; }();
                static const double AFLOPS = [] { const char *e = std::getenv("TLPK_RELAX_AFLOPS"); return e ? std::atof(e) : 1e300; }();
                static const double AGAMMA = [] { const char *e = std::getenv("TLPK_RELAX_AGAMMA"); return e ? std::atof(e) : 0.0; }();
                const bool rule_a = extra_zeros == 0 || width <= 4 || (width <= 16 && newz <= 0.8 * total) ||
                                    (width <= 48 && newz <= 0.1 * total) ||
                                    (newz <= ZFRAC * total && extra_flops <= AFLOPS + AGAMMA * rsc * rsc);
                const bool rule_b = extra_flops < GAMMA * rsc * rsc && extra_zeros < 0.5 * rsc * rsc;
                // a child almost as tall as its parent (a thin front with thousands of rows) ships an
                // update matrix of ~fp^2 entries for a handful of columns: merging pads little
                // (measured: C4 63.7 -> 62.2 ms/step, headline instance 182 -> 172 ms/step, extend-add 30 -> 11 ms;
                // saturates above ~400)
                const bool rule_c = rsc >= TALL_RATIO * fp && extra_flops < GAMMA_TALL * rsc * rsc && extra_zeros < 0.5 * rsc * rsc;
                if (rule_a || rule_b || rule_c) {
                    into[c] = p; cns[p] += nc; cf[p] = fnew; cz[p] = newz; any_merge = true;
                    const i32 *gf; i32 gc;
                    kid_list(c, gf, gc);
                    cand.insert(cand.end(), gf, gf + gc);          // grandchildren now hang off p
                } else {
                    keep.push_back(c);
                }
            }
            kept_ptr[(size_t)p] = (i32)kept.size(); kept_cnt[(size_t)p] = (i32)keep.size();
            kept.insert(kept.end(), keep.begin(), keep.end());
        }
        pt.mark("amalgamation: re-order");
        if (any_merge) {
            auto root_of = [&](i32 s) { while (into[s] != -1) s = into[s]; return s; };
            // members of every group (ascending), flat
            std::vector<i32> grp((size_t)ns_total), mem_ptr((size_t)ns_total + 1, 0), mem((size_t)ns_total);
            for (i32 s = 0; s < ns_total; ++s) { grp[(size_t)s] = root_of(s); mem_ptr[(size_t)grp[(size_t)s] + 1]++; }
            for (i32 s = 0; s < ns_total; ++s) mem_ptr[(size_t)s + 1] += mem_ptr[(size_t)s];
            {
                std::vector<i32> fill(mem_ptr.begin(), mem_ptr.end() - 1);
                for (i32 s = 0; s < ns_total; ++s) mem[(size_t)fill[(size_t)grp[(size_t)s]]++] = s;
            }
            // post-order over the group tree (children groups before the group's own columns)
            std::vector<i32> newpos(m, -1), new_start;
            i32 counter = 0;
            std::vector<std::pair<i32, size_t>> stack;
            for (i32 r = 0; r < ns_total; ++r) {
                if (into[r] != -1 || sparent[r] != -1) continue;     // group roots without a parent
                stack.emplace_back(r, 0);
                while (!stack.empty()) {
                    auto &top = stack.back();
                    const i32 g = top.first;
                    const i32 *kf; i32 kc;
                    kid_list(g, kf, kc);
                    if (top.second < (size_t)kc) { const i32 ch = kf[top.second++]; stack.emplace_back(ch, 0); continue; }
                    new_start.push_back(counter);
                    for (i32 q = mem_ptr[(size_t)g]; q < mem_ptr[(size_t)g + 1]; ++q) {
                        const i32 mm = mem[(size_t)q];
                        for (i32 j = sn_start[mm]; j < sn_start[mm + 1]; ++j) newpos[j] = counter++;
                    }
                    stack.pop_back();
                }
            }
            if (counter != m) return fail(S, TLPK_INTERNAL, "amalgamation re-ordering lost columns");
            new_start.push_back(m);
            std::vector<i32> perm2(m), parent2(m, -1), cc2(m);
            par_chunks(m, [&](i64 lo, i64 hi) {
                for (i64 k = lo; k < hi; ++k) {
                    perm2[newpos[k]] = S.perm[k];
                    cc2[newpos[k]] = S.colcount[k];
                    if (S.parent[k] != -1) parent2[newpos[k]] = newpos[S.parent[k]];
                }
            });
            S.perm.swap(perm2); S.parent.swap(parent2); S.colcount.swap(cc2);
            par_chunks(m, [&](i64 lo, i64 hi) { for (i64 k = lo; k < hi; ++k) S.iperm[S.perm[k]] = (i32)k; });
            {
                std::atomic<int> bad_topo{0};
                par_chunks(m, [&](i64 lo, i64 hi) { for (i64 k = lo; k < hi; ++k) if (S.parent[k] != -1 && S.parent[k] <= k) bad_topo = 1; });
                if (bad_topo) return fail(S, TLPK_INTERNAL, "re-ordered etree not topological");
            }
            if (nlink) for (i32 k = first_link; k < m; ++k) if (!is_link[S.perm[k]]) return fail(S, TLPK_INTERNAL, "linking rows moved");
            sn_start.swap(new_start);
            pt.mark("amalgamation: pattern");
            build_pattern();
        }
        pt.mark("amalgamation: fronts");
        const int rc = build_fronts(true);
        if (rc != TLPK_OK) return rc;
    }
    { std::vector<i32>().swap(adj); std::vector<i64>().swap(xadj); }
    S.nlink_v = nlink;
    pt.mark(nullptr);
    return TLPK_OK;
}

// ---- the products of the assembly lists (step 14 of analyse_rank; build_value_maps) ----
// S[ii,kk] = sum_j A[i,j] D_j A[k,j]: walk_pairs visits the products of pivot column kk (permuted numbering) in the order of the lists -- rows of A' in
// order, entries of the column of A in order -- and hands f(ii, pa, pb, j) the permuted row of the entry, the positions of the two factors in the value array
// of the analysed matrix (the product is value[pa] * value[pb], in this order) and the column of D; pa = pb = -1: the constant -1 on the diagonal of a
// variable node (K2) / a dense-column node.
struct PairWalk {
    const i64 *Ap; const i32 *Ai; const i64 *Tp; const i32 *Tj; const i32 *Tpos; const i32 *perm, *iperm; const char *col_local;
    i32 system; i64 k2_n; i32 rank; i32 dense_m, dense_n; const i64 *dense_cols;
};
template <class F>
static inline void walk_pairs(const PairWalk &W, i32 kk, bool is_root, F &&f) {
    const i32 k = W.perm[kk];
    if (W.system == 1) {
        // Augmented system: the diagonal of a variable node is -(theta + regP) = -1 * D2[k]; an
        // off-diagonal entry is the constant A[i,j] = A[i,j] * D2[k2_n] with D2[k2_n] = 1 (the columns
        // of the incidence matrix carry (1, A[i,j]) on the variable / constraint node).
        // Sharded runs: the assembled entries of the replicated root front (linking constraint nodes and the
        // variable nodes of columns that touch linking rows only) belong to rank 0; the all-reduce of the root
        // panel adds the ranks' extend-add contributions to them.
        if (is_root && W.rank != 0) return;
        if (k < W.k2_n) f(kk, (i64)-1, (i64)-1, k);
        for (i64 q = W.Tp[k]; q < W.Tp[k + 1]; ++q) {
            const i32 j = W.Tj[q];
            const i64 pa = W.Tpos[q];
            for (i64 p = W.Ap[j]; p < W.Ap[j + 1]; ++p) {
                const i32 ii = W.iperm[W.Ai[p]];
                if (ii <= kk) continue;
                f(ii, pa, p, (i32)W.k2_n);
            }
        }
    } else if (W.dense_m >= 0) {
        // K1 with dense columns; D = [sparse j: 1 / (theta + regP), dense j: theta + regP ; 1] (kernels.hip: k_dense_diag).
        //   constraint node: the products A[i,j] A[k,j] D_j of the SPARSE columns (columns [0, dense_n) of the incidence matrix; a dense
        //   column is empty there) and the border entries A[i,j] = A[i,j] * D[dense_n] of the incidence columns (A[i,j] on row i, 1 on node
        //   m + t); dense node m + t: -1 * D[dense_cols[t]] on the diagonal (its border entries come from the constraint nodes, ordered before it)
        if (k >= W.dense_m) f(kk, (i64)-1, (i64)-1, (i32)W.dense_cols[(size_t)(k - W.dense_m)]);
        for (i64 q = W.Tp[k]; q < W.Tp[k + 1]; ++q) {
            const i32 j = W.Tj[q];
            const i64 pa = W.Tpos[q];
            const bool incidence = j >= W.dense_n;
            for (i64 p = W.Ap[j]; p < W.Ap[j + 1]; ++p) {
                const i32 ii = W.iperm[W.Ai[p]];
                if (incidence ? ii <= kk : ii < kk) continue;
                f(ii, pa, p, incidence ? W.dense_n : j);
            }
        }
    } else {
        for (i64 q = W.Tp[k]; q < W.Tp[k + 1]; ++q) {
            const i32 j = W.Tj[q];
            if (is_root && !W.col_local[j]) continue;          // sharded: a column of the root front's products belongs to the rank that owns it
            const i64 pa = W.Tpos[q];
            for (i64 p = W.Ap[j]; p < W.Ap[j + 1]; ++p) {
                const i32 ii = W.iperm[W.Ai[p]];
                if (ii < kk) continue;
                f(ii, pa, p, j);
            }
        }
    }
}

int analyse_rank(Symbolic &S, const Options &opt) {
    PhaseTimer pt;
    AnalysePoolScope pool_scope;
    g_host_thread_div = opt.analyse_div > 0 ? opt.analyse_div : std::max<i32>(1, opt.nranks);
    const i32 m = (i32)S.m, n = (i32)S.n;
    const std::vector<i32> &row_block = S.row_block_v, &col_block = S.col_block_v, &sparent = S.sparent_v;
    const i32 nblocks = S.nblocks, nlink = S.nlink_v, ns_total = S.nsuper;
    if (opt.nranks < 1 || opt.rank < 0 || opt.rank >= opt.nranks) return fail(S, TLPK_BADARG, "bad rank/nranks");
    if (opt.nranks > 1 && row_block.empty()) return fail(S, TLPK_BADARG, "sharding needs row_block (general sparse LPs are single-GPU)");
    const bool have_blocks = !row_block.empty();

    pt.mark("levels");
    // ---- 10. depths, levels ----
    S.depth.assign(ns_total, 0);
    for (i32 s = ns_total - 1; s >= 0; --s) S.depth[s] = (sparent[s] == -1) ? 0 : S.depth[sparent[s]] + 1;
    S.nlevels = 0;
    for (i32 s = 0; s < ns_total; ++s) S.nlevels = std::max(S.nlevels, S.depth[s] + 1);
    S.level_ptr.assign((size_t)S.nlevels + 1, 0);
    for (i32 s = 0; s < ns_total; ++s) S.level_ptr[S.depth[s] + 1]++;
    for (i32 d = 0; d < S.nlevels; ++d) S.level_ptr[d + 1] += S.level_ptr[d];
    S.level_fronts.resize(ns_total);
    {
        std::vector<i32> cur(S.level_ptr.begin(), S.level_ptr.end() - 1);
        for (i32 s = 0; s < ns_total; ++s) S.level_fronts[cur[S.depth[s]]++] = s;
    }

    pt.mark("ownership");
    // ---- 11. ownership (block-angular sharding) ----
    S.front_block.assign(ns_total, -1);
    S.front_local.assign(ns_total, 1);
    S.root_front = (nlink > 0) ? ns_total - 1 : -1;
    std::vector<i32> block_owner(std::max(nblocks, 1), 0);
    if (have_blocks) {
        std::vector<double> bflops(nblocks, 0.0);
        for (i32 s = 0; s < ns_total; ++s) {
            const i32 b = row_block[S.perm[S.fronts[s].col0]];
            S.front_block[s] = b;
            if (b >= 0) {
                const double f = S.fronts[s].f, k = S.fronts[s].ns;
                bflops[b] += k * f * f;     // proportional weight
                if (S.fronts[s].parent != -1 && S.front_block[s] < 0) return fail(S, TLPK_INTERNAL, "linking front below the root");
            } else if (s != S.root_front) return fail(S, TLPK_INTERNAL, "linking column outside the root front");
        }
        // contiguous block ranges balanced by weight: block b goes to the rank whose share of
        // the cumulative weight contains b's midpoint; never more ranks than blocks in use
        double total = 0; for (double f : bflops) total += f;
        double acc = 0;
        for (i32 b = 0; b < nblocks; ++b) {
            i32 r = (total > 0) ? (i32)((acc + 0.5 * bflops[b]) / total * opt.nranks) : (i32)((i64)b * opt.nranks / nblocks);
            r = std::max(0, std::min(r, opt.nranks - 1));
            if (b > 0) r = std::max(r, block_owner[b - 1]);
            block_owner[b] = r;
            acc += bflops[b];
        }
        S.n_local_blocks = 0;
        for (i32 b = 0; b < nblocks; ++b) if (block_owner[b] == opt.rank) S.n_local_blocks++;
        for (i32 s = 0; s < ns_total; ++s) {
            const i32 b = S.front_block[s];
            S.front_local[s] = (b < 0) || (block_owner[b] == opt.rank);
        }
    }

    // stream groups: the diagonal blocks are independent subtrees below the root front; block b runs
    // on stream b % ngroups so that one group's latency-bound steps (potrf/trsm chains, diagonal
    // solves) overlap the other groups' MFMA updates.  General sparse LPs: one group.
    S.ngroups = 1;
    if (have_blocks && nblocks >= 2) {
        // 2 groups x (stream + side stream) = 4 streams = the runtime's default number of hardware
        // queues; more streams share queues and serialise (measured: 2 -> 69.5, 3 -> 75.5, 4 -> 74.3 ms/step on C4)
        S.ngroups = std::min(2, nblocks);
        // a rank of a sharded / multi-device handle that owns few blocks: every launch of a group holds one tile set per block, two groups halve it for
        // nothing to overlap with (round 5, rank-local step of C4 / north-star shape: 8 blocks 12.5 vs 13.0 ms, 12 blocks 25.7 vs 25.7, 16 blocks 18.8 vs
        // 18.9, 25 blocks 42.6 vs 42.0, 32 blocks 30.4 vs 30.1 with one / two groups; results do not depend on the number of groups)
        if (opt.nranks > 1 && S.n_local_blocks <= 8) S.ngroups = 1;
        if (opt.streams > 0) S.ngroups = std::min({opt.streams, MAX_GROUPS, nblocks});
        else if (const char *e = std::getenv("TLPK_STREAMS")) S.ngroups = std::max(1, std::min({std::atoi(e), MAX_GROUPS, nblocks}));
    }
    S.front_group.assign(ns_total, 0);
    for (i32 s = 0; s < ns_total; ++s) if (S.front_block[s] >= 0) S.front_group[s] = S.front_block[s] % S.ngroups;

    // a rank only ever walks its own children: drop the other ranks' block roots from the
    // (replicated) root front's child list
    if (opt.nranks > 1)
        for (i32 s = 0; s < ns_total; ++s) {
            FrontDesc &w = S.fronts[s];
            i32 kept = 0;
            for (i32 t = 0; t < w.nchild; ++t) {
                const i32 c = S.children[w.child_ptr + t];
                if (S.front_local[c]) S.children[w.child_ptr + kept++] = c;
            }
            w.nchild = kept;
        }
    S.col_local.assign(n, 1);
    S.row_local.assign(m, 1);
    if (have_blocks && opt.nranks > 1) {
        for (i32 j = 0; j < n; ++j) {
            const i32 b = col_block[j];
            S.col_local[j] = (b < 0) ? (opt.rank == 0) : (block_owner[b] == opt.rank);
        }
        for (i32 i = 0; i < m; ++i) {
            const i32 b = row_block[i];
            S.row_local[i] = (b < 0) ? 2 : (block_owner[b] == opt.rank);   // 2 = linking (replicated)
        }
    } else if (have_blocks) {
        for (i32 i = 0; i < m; ++i) if (row_block[i] < 0) S.row_local[i] = 2;
    }

    pt.mark("offsets");
    // ---- 12. storage offsets (local fronts only) ----
    S.lval_len = 0; S.uc_len = 0; S.ubuf_len[0] = S.ubuf_len[1] = 0; S.dinv_len = 0;
    for (i32 s = 0; s < ns_total; ++s) {
        FrontDesc &w = S.fronts[s];
        w.ubuf = S.depth[s] & 1;
        if (!S.front_local[s]) { w.lda = w.f; w.loff = -1; w.uoff = -1; w.ucoff = -1; w.dinvoff = -1; continue; }
        // Panel columns of the larger fronts start on 128-byte lines: the kernels stream 64..256 contiguous rows of a
        // column per load, and a misaligned 512-byte segment touches 5 lines instead of 4 (measured: 28 % more
        // fabric traffic in the solve sweeps than algorithmic bytes with ld = f).
        w.lda = (w.f >= LDA_PAD_MIN_F) ? (w.f + 15) / 16 * 16 : w.f;
        if (w.lda != w.f || w.f >= LDA_PAD_MIN_F) S.lval_len = (S.lval_len + 15) / 16 * 16;
        w.loff = S.lval_len; S.lval_len += pk_len(w.lda, w.ns);
        w.ucoff = S.uc_len; S.uc_len += (w.f - w.ns);
        if (w.ns >= NB_IN) S.dinv_len = (S.dinv_len + 15) / 16 * 16;     // the inverted 64 x 64 blocks start on 128-byte lines (trsm_task_dma loads them 16 bytes per lane)
        w.dinvoff = S.dinv_len;
        S.dinv_len += (w.ns >= NB_IN) ? (i64)((w.ns + NB_IN - 1) / NB_IN) * NB_IN * NB_IN : (i64)w.ns * w.ns;
    }
    {
        // update-matrix buffers: ping-pong by depth parity inside each stream group (groups are not
        // level-synchronised with each other, so every group gets its own region of both buffers)
        std::vector<std::array<i64, 2>> gmax(S.ngroups, {0, 0});
        std::vector<i64> off;
        for (i32 d = 0; d < S.nlevels; ++d) {
            off.assign(S.ngroups, 0);
            for (i32 t = S.level_ptr[d]; t < S.level_ptr[d + 1]; ++t) {
                const i32 s = S.level_fronts[t];
                FrontDesc &w = S.fronts[s];
                if (!S.front_local[s]) continue;
                const i64 rs = w.f - w.ns;
                const i32 g = S.front_group[s];
                w.uoff = off[g]; off[g] += rs * rs;           // group-relative for now
            }
            for (i32 g = 0; g < S.ngroups; ++g) gmax[g][d & 1] = std::max(gmax[g][d & 1], off[g]);
        }
        std::array<i64, 2> base = {0, 0};
        std::vector<std::array<i64, 2>> gbase(S.ngroups);
        for (i32 g = 0; g < S.ngroups; ++g) { gbase[g] = base; base[0] += gmax[g][0]; base[1] += gmax[g][1]; }
        S.ubuf_len[0] = base[0]; S.ubuf_len[1] = base[1];
        for (i32 s = 0; s < ns_total; ++s) {
            FrontDesc &w = S.fronts[s];
            if (S.front_local[s]) w.uoff += gbase[S.front_group[s]][S.depth[s] & 1];
        }
    }
    S.flops_panel = 0;
    for (i32 s = 0; s < ns_total; ++s) {
        const double f = S.fronts[s].f, k = S.fronts[s].ns;
        // potrf k^3/3 + trsm (f-k)k^2 + syrk (f-k)^2 k, in flops (multiply-add = 2)
        S.flops_panel += k * k * k / 3.0 + (f - k) * k * k + (f - k) * (f - k) * k;
    }

    // Algorithmic flops of the left-looking MFMA update (k_update), in the CHOLMOD `fl` convention that
    // defines flops_chol = sum_j l_j^2 (l_j = true nnz of column j of L, no amalgamation zeros): column
    // j's l_j^2 flops update the l_j trailing rows; the part whose TARGET column lies in the same
    // NB_OUT-wide block column of the front is done by the potrf / trsm kernels, the rest -- targets in
    // later block columns and in the update matrix, (l_j - r_j)^2 with r_j = columns left in j's block
    // column, itself included -- by k_update.  This is the numerator of bench.py's roofline.frac.
    S.flops_update_alg = 0;
    for (i32 s = 0; s < ns_total; ++s) {
        const FrontDesc &w = S.fronts[s];
        if (!S.front_local[s]) continue;
        for (i32 c = 0; c < w.ns; ++c) {
            const i32 r = std::min((c / NB_OUT + 1) * NB_OUT, w.ns) - c;
            const double l = (double)S.colcount[w.col0 + c] - (double)r;
            if (l > 0) S.flops_update_alg += l * l;
        }
    }

    pt.mark("relative indices");
    // ---- 13. relative indices (below-rows of each front -> position in the parent front) ----
    {
        // offsets first (prefix sum), then every front searches its parent on the host threads
        i64 acc = 0;
        for (i32 s = 0; s < ns_total; ++s) { FrontDesc &w = S.fronts[s]; w.reloff = acc; if (w.parent != -1) acc += w.f - w.ns; }
        S.rel.assign((size_t)acc, 0);
        std::atomic<int> bad{0};
        parallel_for_throw(ns_total, host_threads(ns_total), [&](unsigned, i64 s) {
            const FrontDesc &w = S.fronts[s];
            if (w.parent == -1) return;
            const FrontDesc &p = S.fronts[w.parent];
            i64 qp = p.rowoff, out = w.reloff;
            const i64 qend = p.rowoff + p.f;
            for (i64 q = w.rowoff + w.ns; q < w.rowoff + w.f; ++q) {
                const i32 r = S.rowidx[q];
                while (qp < qend && S.rowidx[qp] < r) ++qp;
                if (qp == qend || S.rowidx[qp] != r) { bad = 1; return; }
                S.rel[out++] = (i32)(qp - p.rowoff);
            }
        }, 64);
        if (bad) return fail(S, TLPK_INTERNAL, "child row missing from parent front");
    }
    // ---- 13a. extend-add lookup: the parent's columns are cut into the ranges of its extend-add workgroups
    // (ea_cols wide from 0 inside the pivot columns, and from ns inside the update-matrix columns); for every
    // range boundary the child stores the first of its columns that lands at or after it, so that a workgroup
    // finds "the child's columns in my range" with two loads instead of two binary searches in HBM.
    {
        // fronts whose panel is formed by k_front_assemble (see fa_min_f above)
        S.front_fa.assign((size_t)ns_total, 0);
        for (i32 s = 0; s < ns_total; ++s) {
            const FrontDesc &w = S.fronts[s];
            if (!S.front_local[s] || w.f < fa_min_f() || w.nchild == 0 || (w.f == 1 && w.ns == 1)) continue;
            double contrib = 0;
            for (i32 t = 0; t < w.nchild; ++t) { const FrontDesc &cd = S.fronts[S.children[w.child_ptr + t]]; const double r = cd.f - cd.ns; contrib += 0.5 * r * r; }
            if (contrib >= fa_density() * 0.5 * (double)w.f * w.f && w.ns >= FA_CW) S.front_fa[(size_t)s] = 1;     // contributions per entry of the front
        }
        i64 acc = 0;
        for (i32 s = 0; s < ns_total; ++s) {
            FrontDesc &w = S.fronts[s];
            w.eatab = -1;
            if (w.parent == -1) continue;
            const FrontDesc &p = S.fronts[w.parent];
            const bool pfa = S.front_fa[(size_t)w.parent];
            if (acc > (i64)INT32_MAX - (ea_nbounds(p, pfa) + 1)) return fail(S, TLPK_TOO_LARGE, "extend-add lookup table exceeds 2^31 entries");
            w.eatab = (i32)acc;
            acc += ea_nbounds(p, pfa);
        }
        S.ea_tab.assign((size_t)acc, 0);
        parallel_for_throw(ns_total, host_threads(ns_total), [&](unsigned, i64 s) {
            const FrontDesc &w = S.fronts[s];
            if (w.parent == -1) return;
            const FrontDesc &p = S.fronts[w.parent];
            const bool pfa = S.front_fa[(size_t)w.parent];
            const i32 rsc = w.f - w.ns, nb = ea_nbounds(p, pfa);
            const i32 *rel = S.rel.data() + w.reloff;
            i32 q = 0;
            for (i32 k = 0; k < nb; ++k) {
                const i32 bound = ea_bound(p, pfa, k);
                while (q < rsc && rel[q] < bound) ++q;
                S.ea_tab[(size_t)w.eatab + k] = q;
            }
        }, 64);
    }
    // ---- 13a'. per-column extend-add index (k_ea_gather): the inverse of rel.  A column tc of a selected parent is cut into SEGMENTS of at most
    // ea_gather_cap rows from its diagonal down (rows [tc + p cap, tc + (p + 1) cap) of the front: what one wave holds in LDS); for every segment the
    // (child, child column q) pairs with rel[q] == tc that have rows in it, with those rows, children in the order of the child list -- the summation
    // order of k_extend_add --, so that the wave knows a segment's contributors before its first load.  A segment nothing lands in has no entries and
    // is neither read nor written.  TLPK_EA_GATHER = 0 | 1 | unset (auto), read per analysis: 1 selects every local parent with at least
    // TLPK_EA_GATHER_MIN_CHILD children, auto only those of at least EG_AUTO_MIN_F rows that their children fill densely enough (below).
    // TLPK_EA_GATHER_CAP: rows of a segment.
    {
        constexpr i32 EG_AUTO_MIN_F = 2048; constexpr double EG_AUTO_COLS = 4.0, EG_AUTO_FILL = 4.0;
        int mode = -1; i32 min_child = 16, cap = EG_CAP_MAX;
        if (const char *e = std::getenv("TLPK_EA_GATHER")) mode = std::atoi(e) != 0;
        if (const char *e = std::getenv("TLPK_EA_GATHER_MIN_CHILD")) min_child = (i32)std::max(1, std::atoi(e));
        if (const char *e = std::getenv("TLPK_EA_GATHER_CAP")) cap = (i32)std::max(1, std::min(std::atoi(e), EG_CAP_MAX));
        S.ea_gather_base.assign((size_t)ns_total, -1);
        S.ea_gather_col.clear(); S.ea_gather_ptr.clear(); S.ea_gather_ent.clear();
        S.ea_gather_cap = cap;
        std::vector<i32> sel;
        i64 ncol = 0;
        for (i32 s = 0; s < ns_total && mode != 0; ++s) {
            const FrontDesc &w = S.fronts[s];
            if (!S.front_local[s] || S.front_fa[(size_t)s] || w.nchild < min_child) continue;
            if (mode < 0) {
                // auto: big parents that many thin children hit all over -- on average at least EG_AUTO_COLS child columns per parent column and one child
                // entry per EG_AUTO_FILL entries of the parent's lower triangle.  Below that most of a column that is read and written whole receives
                // nothing, and the scattered adds of k_extend_add move less (measured: DESIGN.md section 5c)
                double cols = 0, ents = 0;
                for (i32 t = 0; t < w.nchild; ++t) { const FrontDesc &cd = S.fronts[S.children[w.child_ptr + t]]; const double r = cd.f - cd.ns; cols += r; ents += 0.5 * r * (r + 1); }
                if (w.f < EG_AUTO_MIN_F || cols < EG_AUTO_COLS * (double)w.f || EG_AUTO_FILL * ents < 0.5 * (double)w.f * (w.f + 1)) continue;
            }
            S.ea_gather_base[(size_t)s] = ncol; ncol += w.f + 1;
            sel.push_back(s);
        }
        // per selected front, on the host threads: the first segment of every column (front-relative), entries per segment, the entries
        struct Part { std::vector<i64> col, ptr; std::vector<EaGatherEnt> ent; };
        std::vector<Part> parts(sel.size());
        parallel_for_throw((i64)sel.size(), host_threads((i64)sel.size()), [&](unsigned, i64 k) {
            const FrontDesc &w = S.fronts[sel[(size_t)k]];
            Part &P = parts[(size_t)k];
            P.col.assign((size_t)w.f + 1, 0);
            for (i32 tc = 0; tc < w.f; ++tc) P.col[(size_t)tc + 1] = P.col[(size_t)tc] + (w.f - tc + cap - 1) / cap;
            const i64 nseg = P.col[(size_t)w.f];
            std::vector<std::pair<i64, EaGatherEnt>> tmp;
            P.ptr.assign((size_t)nseg + 1, 0);
            for (i32 t = 0; t < w.nchild; ++t) {
                const i32 c = S.children[w.child_ptr + t];
                const FrontDesc &cd = S.fronts[c];
                const i32 rsc = cd.f - cd.ns;
                const i32 *rel = S.rel.data() + cd.reloff;
                for (i32 q = 0; q < rsc; ++q) {
                    const i32 tc = rel[q];
                    for (i32 ra = q; ra < rsc;) {              // the child's rows [ra, rb) land in segment pc of column tc
                        const i32 pc = (rel[ra] - tc) / cap;
                        const i32 rb = (i32)(std::lower_bound(rel + ra, rel + rsc, tc + (pc + 1) * cap) - rel);
                        const i64 seg = P.col[(size_t)tc] + pc;
                        tmp.push_back({seg, EaGatherEnt{(cd.uoff + (i64)q * rsc + ra) | ((i64)cd.ubuf << EG_UBUF_BIT), cd.reloff + ra, rb - ra, c}});
                        P.ptr[(size_t)seg + 1]++;
                        ra = rb;
                    }
                }
            }
            for (i64 g = 0; g < nseg; ++g) P.ptr[(size_t)g + 1] += P.ptr[(size_t)g];
            std::vector<i64> fill(P.ptr.begin(), P.ptr.end() - 1);
            P.ent.resize(tmp.size());
            for (const auto &te : tmp) P.ent[(size_t)fill[(size_t)te.first]++] = te.second;      // (stable: child order inside a segment)
        });
        i64 nseg = 0, nent = 0;
        for (const Part &P : parts) { nseg += (i64)P.ptr.size() - 1; nent += (i64)P.ent.size(); }
        if (!sel.empty()) {
            S.ea_gather_col.reserve((size_t)ncol); S.ea_gather_ptr.reserve((size_t)nseg + 1); S.ea_gather_ent.reserve((size_t)nent);
            i64 seg0 = 0, ent0 = 0;
            for (const Part &P : parts) {
                for (const i64 v : P.col) S.ea_gather_col.push_back(seg0 + v);
                for (size_t g = 0; g + 1 < P.ptr.size(); ++g) S.ea_gather_ptr.push_back(ent0 + P.ptr[g]);
                S.ea_gather_ent.insert(S.ea_gather_ent.end(), P.ent.begin(), P.ent.end());
                seg0 += (i64)P.ptr.size() - 1; ent0 += (i64)P.ent.size();
            }
            S.ea_gather_ptr.push_back(ent0);
        }
    }

    pt.mark("structural zeros");
    // ---- 13c. structural zeros of the amalgamated fronts.  A merged supernode is stored and factorised as a dense trapezoid, but
    // the columns of an absorbed child are zero outside the child's own row structure: on the north-star instance a third of the
    // flops of the left-looking update multiplied such zeros.  For every front with padding: one bit per (16-column K slab, 16-row
    // group) = "some column of the slab has a TRUE nonzero of L in these rows"; build_schedule gives every update tile the list of
    // K slabs in which BOTH of its operand row ranges have one.  True structures come from the column elimination tree: inside a front the
    // columns form chains with nested structures (parent[j-1] == j and count[j-1] == count[j] + 1: struct(j) = struct(j-1) \ {j-1}), the
    // structure of a chain head is its column of S, the structures of the etree children of the chain's columns that lie in the front,
    // and the rows below the child FRONTS that enter the front at a column of the chain (the last column of a front holds all rows
    // below the front).  Bits of rows above a column are never consulted (operand rows lie below the K columns), so plain ORs do.
    {
        i64 min_f = 256;
        bool on = true;
        if (const char *e = std::getenv("TLPK_SKIP")) on = std::atoi(e) != 0;                  // TLPK_SKIP=0: no skip lists
        if (const char *e = std::getenv("TLPK_SKIP_MIN_F")) min_f = std::atoll(e);             // testing knob
        S.skip_off.assign((size_t)ns_total, -1);
        S.skip_bits.clear();
        std::vector<i32> elig;
        i64 acc = 0;
        if (on)
            for (i32 s = 0; s < ns_total; ++s) {
                const FrontDesc &w = S.fronts[s];
                if (!S.front_local[s] || w.ns < 2 * 16 || w.f < min_f || w.f <= w.ns) continue;
                i64 stored = 0, truth = 0;
                for (i32 c = 0; c < w.ns; ++c) { stored += w.f - c; truth += S.colcount[w.col0 + c]; }
                if (stored == truth) continue;                 // no padding: nothing to skip
                const i64 nsl = (w.ns + 15) / 16, W = ((w.f + 15) / 16 + 63) / 64;
                S.skip_off[s] = acc; acc += nsl * W;
                elig.push_back(s);
            }
        S.skip_bits.assign((size_t)acc, 0);
        std::atomic<int> bad{0};
        parallel_for_throw((i64)elig.size(), host_threads((i64)elig.size()), [&](unsigned, i64 q) {
            const i32 s = elig[(size_t)q];
            const FrontDesc &w = S.fronts[s];
            const i32 ns = w.ns, f = w.f, col0 = w.col0;
            const i64 W = ((f + 15) / 16 + 63) / 64;
            std::vector<i32> head(ns), hid(ns, -1);
            i32 nheads = 0;
            for (i32 c = 0; c < ns; ++c) {
                const bool chain = c > 0 && S.parent[col0 + c - 1] == col0 + c && S.colcount[col0 + c - 1] == S.colcount[col0 + c] + 1;
                head[c] = chain ? head[c - 1] : c;
                if (!chain) hid[c] = nheads++;
            }
            std::vector<uint64_t> B((size_t)nheads * W, 0);
            auto setpos = [&](uint64_t *b, i32 pos) { b[(pos >> 4) >> 6] |= (uint64_t)1 << ((pos >> 4) & 63); };
            const i32 *below = S.rowidx.data() + w.rowoff + ns;
            for (i32 t = 0; t < w.nchild; ++t) {
                const FrontDesc &cd = S.fronts[S.children[w.child_ptr + t]];
                const i32 p = S.parent[cd.col0 + cd.ns - 1];
                if (p < col0 || p >= col0 + ns) { bad = 1; return; }
                uint64_t *hb = B.data() + (size_t)hid[head[p - col0]] * W;
                for (i32 r = 0; r < cd.f - cd.ns; ++r) setpos(hb, S.rel[cd.reloff + r]);
            }
            for (i32 c = 0; c < ns; ++c) {
                const i32 j = col0 + c;
                uint64_t *hb = B.data() + (size_t)hid[head[c]] * W;
                if (head[c] == c)
                    for (i64 e = S.Sp[j]; e < S.Sp[j + 1]; ++e) {
                        const i32 i = S.Si[e];
                        i32 pos;
                        if (i < col0 + ns) pos = i - col0;
                        else {
                            const i32 *it = std::lower_bound(below, below + (f - ns), i);
                            if (it == below + (f - ns) || *it != i) { bad = 1; return; }
                            pos = ns + (i32)(it - below);
                        }
                        setpos(hb, pos);
                    }
                const i32 p = S.parent[j];
                if (p != -1 && p < col0 + ns && head[p - col0] != head[c]) {
                    uint64_t *pb = B.data() + (size_t)hid[head[p - col0]] * W;
                    for (i64 x = 0; x < W; ++x) pb[x] |= hb[x];
                }
            }
            uint64_t *out = S.skip_bits.data() + S.skip_off[s];
            for (i32 c = 0; c < ns; ++c) {
                if (c > 0 && head[c] == head[c - 1] && (c & 15) != 0) continue;      // same chain as the previous column of this slab
                const uint64_t *hb = B.data() + (size_t)hid[head[c]] * W;
                uint64_t *ob = out + (size_t)(c >> 4) * W;
                for (i64 x = 0; x < W; ++x) ob[x] |= hb[x];
            }
        }, 1);
        if (bad) return fail(S, TLPK_INTERNAL, "structural-zero analysis: inconsistent front structure");
    }

    pt.mark("gather lists");
    // ---- 13b. forward-solve gather lists: for every row t of a front, the entries of its
    // children's contribution vectors that land on it, in child order (the order the sums are
    // taken in).  One thread per row then gathers without conflicts.
    {
        const i64 nrow_total = (i64)S.rowidx.size();
        S.gth_ptr.assign(nrow_total + 1, 0);
        const unsigned nthreads = host_threads(ns_total);
        // the rows [rowoff, rowoff + f) of a front belong to that front alone: fronts on the host threads
        parallel_for_throw(ns_total, nthreads, [&](unsigned, i64 s) {
            const FrontDesc &w = S.fronts[s];
            if (!S.front_local[s]) return;
            for (i32 t = 0; t < w.nchild; ++t) {
                const FrontDesc &cd = S.fronts[S.children[w.child_ptr + t]];
                const i32 rsc = cd.f - cd.ns;
                for (i32 r = 0; r < rsc; ++r) ++S.gth_ptr[w.rowoff + S.rel[cd.reloff + r] + 1];
            }
        }, 64);
        for (i64 i = 0; i < nrow_total; ++i) S.gth_ptr[i + 1] += S.gth_ptr[i];
        S.gth_src.assign(S.gth_ptr[nrow_total], 0);
        std::vector<i64> cur(S.gth_ptr.begin(), S.gth_ptr.end() - 1);
        parallel_for_throw(ns_total, nthreads, [&](unsigned, i64 s) {
            const FrontDesc &w = S.fronts[s];
            if (!S.front_local[s]) return;
            for (i32 t = 0; t < w.nchild; ++t) {
                const FrontDesc &cd = S.fronts[S.children[w.child_ptr + t]];
                const i32 rsc = cd.f - cd.ns;
                for (i32 r = 0; r < rsc; ++r) S.gth_src[cur[w.rowoff + S.rel[cd.reloff + r]]++] = cd.ucoff + r;
            }
        }, 64);
    }
    pt.mark("assembly lists");
    // ---- 14. assembly lists: S[ii,kk] = sum_j A[i,j] D_j A[k,j] (+ regD on the diagonal) ----
    {
        // (uvec: no zero-fill by resize; the defaults are written by the host threads, chunk by chunk)
        S.s_target.resize((size_t)S.nnzS); S.s_diag_row.resize((size_t)S.nnzS); S.s_local.resize((size_t)S.nnzS); S.pair_ptr.resize((size_t)S.nnzS + 1);
        {
            constexpr i64 CH = (i64)1 << 16;
            const i64 nch = (S.nnzS + CH) / CH;                  // covers pair_ptr[nnzS]
            if (!parallel_for(nch, host_threads(nch), [&](unsigned, i64 ch) {
                    const i64 e0 = ch * CH, e1 = std::min(S.nnzS, e0 + CH);
                    for (i64 e = e0; e < e1; ++e) { S.s_target[(size_t)e] = -1; S.s_diag_row[(size_t)e] = -1; S.s_local[(size_t)e] = 0; S.pair_ptr[(size_t)e] = 0; }
                    if (e1 == S.nnzS) S.pair_ptr[(size_t)S.nnzS] = 0;
                })) return fail(S, TLPK_OOM, "out of memory while building the assembly lists");
        }
        pt.mark("assembly lists: traverse");
        // Round 6: ONE traversal of A per pivot column instead of two (count, then fill).  Fronts are independent (every stored entry of S belongs to exactly one
        // pivot column of exactly one front): handed out to the host threads.  A thread walks the products of a column once -- the order of the old fill pass:
        // rows of A' in order, entries of the column of A in order --, groups them by entry of S with a stable counting sort inside the column (a few hundred
        // products: cache-resident) and appends the column to its own stream; the counts go to pair_ptr.  After the prefix sum every column is ONE contiguous
        // copy from its thread's stream to its final place.  The lists are the lists of the two-pass version, entry by entry (tests/test_symbolic.py: digests).
        const unsigned nthreads = host_threads(ns_total);
        // K1 with dense columns: constraint nodes [0, dense_m); the incidence matrix's columns [0, dense_n) are A's (the dense ones empty)
        const i32 dense_m = S.n_dense > 0 ? m - (i32)S.n_dense : -1;
        const i32 dense_n = (i32)S.dense_n;
        const PairWalk W{S.Ap.data(), S.Ai.data(), S.Tp.data(), S.Tj.data(), S.Tpos.data(), S.perm.data(), S.iperm.data(), S.col_local.data(),
                         opt.system, opt.k2_n, opt.rank, dense_m, dense_n, S.dense_cols.data()};
        struct Stream { std::vector<double> w; std::vector<i32> j; std::vector<i32> le, cj, start; std::vector<double> cw; std::vector<i32> pos_in_front; std::vector<i64> epos; };
        std::vector<Stream> st(nthreads);
        uvec<i64> col_off((size_t)m);                     // per pivot column: offset of its products in the stream of ...
        uvec<i32> col_thr((size_t)m);                     // ... this thread (-1: a column of a front this rank does not own)
        {
            const bool ok = parallel_for(ns_total, nthreads, [&](unsigned tid, i64 s64) {
                const i32 s = (i32)s64;
                const FrontDesc &w = S.fronts[s];
                if (!S.front_local[s]) { for (i32 kk = w.col0; kk < w.col0 + w.ns; ++kk) col_thr[(size_t)kk] = -1; return; }
                Stream &T = st[tid];
                if (T.pos_in_front.empty()) { T.pos_in_front.assign(m, -1); T.epos.assign(m, -1); }
                std::vector<i32> &pos_in_front = T.pos_in_front;
                std::vector<i64> &epos = T.epos;
                const bool is_root = (s == S.root_front);
                for (i32 t = 0; t < w.f; ++t) pos_in_front[S.rowidx[w.rowoff + t]] = t;
                for (i32 kk = w.col0; kk < w.col0 + w.ns; ++kk) {
                    const i32 k = S.perm[kk];
                    const i64 e0 = S.Sp[kk], ne = S.Sp[kk + 1] - e0;
                    for (i64 e = e0; e < e0 + ne; ++e) {
                        const i32 ii = S.Si[e];
                        epos[ii] = e;
                        S.s_target[e] = w.loff + pos_in_front[ii] + pk_off(w.lda, kk - w.col0);
                        S.s_local[e] = 1;
                    }
                    if (opt.system == 1) { if (k >= opt.k2_n && (!is_root || opt.rank == 0)) S.s_diag_row[e0] = k - (i32)opt.k2_n; }   // constraint node: regD
                    else if (dense_m >= 0) { if (k < dense_m) S.s_diag_row[e0] = k; }                                        // dense node: no regD
                    else if (!is_root || opt.rank == 0) S.s_diag_row[e0] = k;
                    T.le.clear(); T.cw.clear(); T.cj.clear();
                    T.start.assign((size_t)ne + 1, 0);
                    auto emit = [&](i64 e, double wv, i32 j) { const i32 le = (i32)(e - e0); T.le.push_back(le); T.cw.push_back(wv); T.cj.push_back(j); ++T.start[(size_t)le + 1]; };
                    // (the walk is shared with build_value_maps: the same products in the same order, the factors in the same order)
                    walk_pairs(W, kk, is_root, [&](i32 ii, i64 pa, i64 pb, i32 j) { emit(epos[ii], pa < 0 ? -1.0 : S.Ax[(size_t)pa] * S.Ax[(size_t)pb], j); });
                    // counts -> pair_ptr (prefix-summed below); stable counting sort of the column's products by entry into the thread's stream
                    const size_t np = T.le.size(), base = T.w.size();
                    for (i64 q = 0; q < ne; ++q) { S.pair_ptr[(size_t)(e0 + q) + 1] = T.start[(size_t)q + 1]; T.start[(size_t)q + 1] += T.start[(size_t)q]; }
                    T.w.resize(base + np); T.j.resize(base + np);
                    for (size_t q = 0; q < np; ++q) { const size_t at = base + (size_t)T.start[(size_t)T.le[q]]++; T.w[at] = T.cw[q]; T.j[at] = T.cj[q]; }
                    col_off[(size_t)kk] = (i64)base; col_thr[(size_t)kk] = (i32)tid;
                }
            }, 64);
            if (!ok) return fail(S, TLPK_OOM, "out of memory while building the assembly lists");
        }
        pt.mark("assembly lists: prefix");
        {
            // prefix sum in two levels: per chunk of 65 536 entries on the host threads, the chunk totals serially
            constexpr i64 CH = (i64)1 << 16;
            const i64 nch = (S.nnzS + CH - 1) / CH;
            std::vector<i64> tot((size_t)nch + 1, 0);
            bool ok = parallel_for(nch, host_threads(nch), [&](unsigned, i64 ch) {
                const i64 a = ch * CH, b = std::min(S.nnzS, a + CH);
                i64 acc = 0;
                for (i64 e = a; e < b; ++e) { acc += S.pair_ptr[(size_t)e + 1]; S.pair_ptr[(size_t)e + 1] = acc; }
                tot[(size_t)ch + 1] = acc;
            });
            for (i64 ch = 0; ch < nch; ++ch) tot[(size_t)ch + 1] += tot[(size_t)ch];
            ok = ok && parallel_for(nch, host_threads(nch), [&](unsigned, i64 ch) {
                const i64 a = ch * CH, b = std::min(S.nnzS, a + CH), add = tot[(size_t)ch];
                if (add) for (i64 e = a; e < b; ++e) S.pair_ptr[(size_t)e + 1] += add;
            });
            if (!ok) return fail(S, TLPK_OOM, "out of memory while building the assembly lists");
            S.pair_ptr[0] = 0;
        }
        pt.mark("assembly lists: place");
        {
            S.pair_w.resize((size_t)S.pair_ptr[S.nnzS]); S.pair_j.resize((size_t)S.pair_ptr[S.nnzS]);      // (first touched by the threads that fill them)
            const bool ok = parallel_for(m, host_threads(m / 256 + 1), [&](unsigned, i64 kk) {
                const i32 th = col_thr[(size_t)kk];
                if (th < 0) return;
                const i64 a = S.pair_ptr[(size_t)S.Sp[kk]], cnt = S.pair_ptr[(size_t)S.Sp[kk + 1]] - a;
                if (cnt <= 0) return;
                std::memcpy(S.pair_w.data() + a, st[(size_t)th].w.data() + col_off[(size_t)kk], (size_t)cnt * sizeof(double));
                std::memcpy(S.pair_j.data() + a, st[(size_t)th].j.data() + col_off[(size_t)kk], (size_t)cnt * sizeof(i32));
            }, 256);
            if (!ok) return fail(S, TLPK_OOM, "out of memory while building the assembly lists");
        }
    }
    pt.mark("schedule");
    S.error.clear();
    S.shared_device = opt.shared_device;
    build_schedule(S);
    if (!S.error.empty()) return TLPK_INTERNAL;
    // k_update walks its K range in slabs of 16 columns and relies on a slab lying inside ONE 64-column slice of the packed panel
    for (const UpdateTask &u : S.update_tasks)
        if ((u.k0 & 15) != 0) return fail(S, TLPK_INTERNAL, "update task: K range does not start on a multiple of 16 columns");
    // ---- 14'. formed fronts (TLPK_EA_FORM = 0 | 1, unset = 1).  A gathered front whose panel columns all belong to k_ea_gather -- its
    // extend-add tasks cover [0, ns) and none of them is a row band (TLPK_EA_BANDS) -- needs no zero-fill: the kernel starts a segment from zeros and the
    // entries of S that k_assemble has stored in it, and writes every stored double of the column.  For that it needs the rows of those entries per segment:
    // from the assembly targets and the packed layout, ascending.  After the schedule (the tasks decide), and nothing the schedule digest covers moves.
    S.ea_form.clear(); S.ea_gather_asm_ptr.clear(); S.ea_gather_asm_row.clear();
    {
        bool on = true;
        if (const char *e = std::getenv("TLPK_EA_FORM")) on = std::atoi(e) != 0;
        const size_t nf = S.fronts.size();
        std::vector<unsigned char> form(nf, 0);
        bool any = false;
        if (on && !S.ea_gather_ent.empty()) {
            std::vector<i64> covered(nf, 0);
            std::vector<char> banded(nf, 0);
            for (const EaTask &t : S.ea_tasks) {
                if (S.ea_gather_base[(size_t)t.front] < 0) continue;
                if (t.br1 != 0) banded[(size_t)t.front] = 1;
                else if (t.j1 <= S.fronts[(size_t)t.front].ns) covered[(size_t)t.front] += t.j1 - t.j0;
            }
            for (size_t s = 0; s < nf; ++s)
                if (S.ea_gather_base[s] >= 0 && !S.front_fa[s] && !banded[s] && covered[s] == S.fronts[s].ns) { form[s] = 1; any = true; }
        }
        if (any) {
            const i32 cap = S.ea_gather_cap;
            const i64 nseg = (i64)S.ea_gather_ptr.size() - 1;
            std::vector<i64> &ptr = S.ea_gather_asm_ptr;
            ptr.assign((size_t)nseg + 1, 0);
            // two passes over the entries of the formed fronts' pivot columns: count per segment, then place
            for (int pass = 0; pass < 2; ++pass) {
                std::vector<i64> fill;
                if (pass == 1) {
                    for (i64 g = 0; g < nseg; ++g) ptr[(size_t)g + 1] += ptr[(size_t)g];
                    S.ea_gather_asm_row.assign((size_t)ptr[(size_t)nseg], 0);
                    fill.assign(ptr.begin(), ptr.end() - 1);
                }
                for (size_t s = 0; s < nf; ++s) {
                    if (!form[s]) continue;
                    const FrontDesc &w = S.fronts[s];
                    const i64 *colseg = S.ea_gather_col.data() + S.ea_gather_base[s];
                    for (i32 tc = 0; tc < w.ns; ++tc) {
                        const i64 kk = (i64)w.col0 + tc, vrow0 = w.loff + pk_off(w.lda, tc);
                        for (i64 e = S.Sp[(size_t)kk]; e < S.Sp[(size_t)kk + 1]; ++e) {
                            const i64 row = S.s_target[(size_t)e] - vrow0;
                            if (!S.s_local[(size_t)e] || row < tc || row >= w.f) return fail(S, TLPK_INTERNAL, "formed front: an assembly target outside its panel column");
                            const i64 pc = (row - tc) / cap, g = colseg[tc] + pc;
                            if (pass == 0) ptr[(size_t)g + 1]++;
                            else S.ea_gather_asm_row[(size_t)fill[(size_t)g]++] = (uint16_t)(row - tc - pc * cap);
                        }
                    }
                }
            }
            for (i64 g = 0; g < nseg; ++g) std::sort(S.ea_gather_asm_row.begin() + ptr[(size_t)g], S.ea_gather_asm_row.begin() + ptr[(size_t)g + 1]);
            S.ea_form = std::move(form);
        }
    }
    // ---- 14''. flat segment list of the formed fronts' panel columns (TLPK_EA_SEGLIST = 0 | 1, unset = 1).  k_ea_gather<true> reaches a
    // segment through task -> FrontDesc -> eg_base -> eg_col -> eg_ptr / asm_ptr, a chain of dependent loads per column; the list spells every segment out --
    // where it is stored, its rows, its contributors, its assembled rows, what its column zeroes besides -- in the order the launches, their tasks, the tasks'
    // columns and the columns' segments come, so that a wave of k_ea_seglist walks a run of consecutive records and fetches ahead across segments and columns.
    // Per launch with such tasks the range of its records.  Nothing else moves; 0 builds no list and keeps the task-driven kernel.
    S.ea_seg.clear(); S.ea_seg_launch.clear();
    {
        bool on = true;
        if (const char *e = std::getenv("TLPK_EA_SEGLIST")) on = std::atoi(e) != 0;
        if (on && !S.ea_form.empty()) {
            const i32 cap = S.ea_gather_cap;
            for (const Launch &L : S.factor_launches) {
                if (L.kind != LK_EXTEND_ADD || L.count <= 0) continue;
                const i64 s0 = (i64)S.ea_seg.size();
                for (i64 k = L.first; k < L.first + L.count; ++k) {
                    const EaTask &t = S.ea_tasks[(size_t)k];
                    const FrontDesc &w = S.fronts[(size_t)t.front];
                    if (!S.ea_form[(size_t)t.front] || t.br1 != 0 || t.j0 >= w.ns) continue;        // (kernels.hip: ea_task_gathered, ea_task_formed)
                    if (w.lda - w.f > UINT16_MAX) return fail(S, TLPK_INTERNAL, "formed front: padding rows do not fit a segment record");
                    const i64 *colseg = S.ea_gather_col.data() + S.ea_gather_base[(size_t)t.front];
                    for (i32 tc = t.j0; tc < t.j1; ++tc) {
                        const i64 g0 = colseg[tc], g1 = colseg[tc + 1], vrow0 = w.loff + pk_off(w.lda, tc);
                        for (i64 g = g0; g < g1; ++g) {
                            const i32 r0 = tc + (i32)(g - g0) * cap, n = std::min(cap, w.f - r0);
                            const i64 e0 = S.ea_gather_ptr[(size_t)g], ne = S.ea_gather_ptr[(size_t)g + 1] - e0;
                            const i64 a0 = S.ea_gather_asm_ptr[(size_t)g], na = S.ea_gather_asm_ptr[(size_t)g + 1] - a0;
                            if (ne > INT32_MAX) return fail(S, TLPK_TOO_LARGE, "formed front: a segment has more than 2^31 contributors");
                            // (k_ea_seglist walks a batch's contributors with a cursor that relies on every one having a row: step 13a' makes no other)
                            for (i64 q = e0; q < e0 + ne; ++q)
                                if (S.ea_gather_ent[(size_t)q].n < 1) return fail(S, TLPK_INTERNAL, "formed front: a contributor without rows in the segment list");
                            S.ea_seg.push_back(EaSeg{vrow0 + r0, e0, a0, t.front, r0, (i32)ne, (uint16_t)n, (uint16_t)na, (uint16_t)(g == g0 ? (tc & 63) : 0),
                                                     (uint16_t)(g + 1 == g1 ? w.lda - w.f : 0), 0});
                        }
                    }
                }
                if ((i64)S.ea_seg.size() > s0) S.ea_seg_launch.push_back(EaSegLaunch{L.first, s0, (i64)S.ea_seg.size()});
            }
        }
    }
    pt.mark(nullptr);
    return TLPK_OK;
}

int analyse(Symbolic &S, i64 m, i64 n, const i64 *colptr, const i64 *rowval, const double *nzval, int base, const Options &opt) {
    const int rc = analyse_common(S, m, n, colptr, rowval, nzval, base, opt);
    return rc != TLPK_OK ? rc : analyse_rank(S, opt);
}

// ---------------------------------------------------------------------------------------------
// K2: the augmented system K = [-(Theta^-1 + Rp)  A'; A  Rd] of order N = n + m
// (/root/reference/src/KKT/KKT.jl:70-75, src/KKT/Cholmod/sqd.jl:5-74, src/KKT/LDLFactorizations/ldlfact.jl:63-139).
// K is symmetric quasi-definite: any symmetric permutation has a factorisation P K P' = L S L' with
// S = diag(+-1) known in advance (-1 for a variable node, +1 for a constraint node) and no pivoting
// (Vanderbei 1995), i.e. a "signed Cholesky" that runs on the same supernodal machinery.  The graph
// of K is the graph of B B' for the N x nnz(A) incidence matrix B whose column p holds 1 on the
// variable node and A[i,j] on the constraint node of the p-th nonzero of A: the whole analyse phase is
// reused on B, only the assembly lists differ (see step 14).
// ---------------------------------------------------------------------------------------------
// rank-independent part: incidence matrix, analyse_common on it, signs
int analyse_k2_common(Symbolic &S, i64 m, i64 n, const i64 *colptr, const i64 *rowval, const double *nzval,
                      int base, const Options &opt_in, Options *opt_out) {
    if (m < 0 || n < 0 || (base != 0 && base != 1) || !colptr) return fail(S, TLPK_BADARG, "bad dimensions or index base");
    const i64 nnz = colptr[n] - base;
    if (nnz < 0 || m + n >= ((i64)1 << 31) || nnz >= ((i64)1 << 30)) return fail(S, TLPK_TOO_LARGE, "augmented system exceeds int32");
    if (nnz > 0 && (!rowval || !nzval)) return fail(S, TLPK_BADARG, "null rowval/nzval");
    std::vector<i64> bp((size_t)nnz + 1), bi((size_t)(2 * nnz));
    std::vector<double> bx((size_t)(2 * nnz));
    for (i64 j = 0; j < n; ++j) {
        if (colptr[j] - base < 0 || colptr[j + 1] < colptr[j] || colptr[j + 1] - base > nnz) return fail(S, TLPK_BADARG, "colptr not monotone");
        for (i64 p = colptr[j] - base; p < colptr[j + 1] - base; ++p) {
            const i64 r = rowval[p] - base;
            if (r < 0 || r >= m) return fail(S, TLPK_BADARG, "row index out of range");
            bp[(size_t)p] = 2 * p;
            bi[(size_t)(2 * p)] = j; bx[(size_t)(2 * p)] = 1.0;                  // variable node
            bi[(size_t)(2 * p + 1)] = n + r; bx[(size_t)(2 * p + 1)] = nzval[p];   // constraint node
        }
    }
    bp[(size_t)nnz] = 2 * nnz;
    Options opt = opt_in;
    opt.system = 1; opt.k2_n = n;
    // Block-angular LPs: the nodes of the augmented system inherit the blocks of the rows -- constraint node n + i that of
    // row i, variable node j that of the diagonal-block rows its column touches (a column with entries in linking rows
    // only, e.g. a linking row's slack, joins the linking nodes: -1 = root front).  Ordering per block, stream groups and
    // the root front then work as for K1; the root mixes both signs, which the signed Cholesky does not mind.
    std::vector<i64> node_block;
    if (opt_in.row_block) {
        node_block.assign((size_t)(m + n), -1);
        for (i64 i = 0; i < m; ++i) node_block[(size_t)(n + i)] = opt_in.row_block[i];
        for (i64 j = 0; j < n; ++j) {
            i64 b = -1;
            for (i64 p = colptr[j] - base; p < colptr[j + 1] - base; ++p) {
                const i64 rb = opt_in.row_block[rowval[p] - base];
                if (rb < 0) continue;
                if (b >= 0 && rb != b) return fail(S, TLPK_BADARG, "row_block is not a block-angular partition: a column couples two diagonal blocks");
                b = rb;
            }
            node_block[(size_t)j] = b;
        }
        opt.row_block = node_block.data();
    }
    const int rc = analyse_common(S, m + n, nnz, bp.data(), bi.data(), bx.data(), 0, opt);
    if (rc != TLPK_OK) return rc;
    S.system = 1; S.k2_n = n; S.k2_m = m;
    S.csign.resize((size_t)(m + n));
    for (i64 kk = 0; kk < m + n; ++kk) S.csign[(size_t)kk] = (S.perm[(size_t)kk] < n) ? -1.0 : 1.0;
    opt.row_block = nullptr;                    // (points into a local; analyse_rank reads the copy inside S)
    if (opt_out) *opt_out = opt;
    return TLPK_OK;
}

int analyse_k2(Symbolic &S, i64 m, i64 n, const i64 *colptr, const i64 *rowval, const double *nzval,
               int base, const Options &opt_in) {
    Options opt;
    const int rc = analyse_k2_common(S, m, n, colptr, rowval, nzval, base, opt_in, &opt);
    return rc != TLPK_OK ? rc : analyse_rank(S, opt);
}

// ---------------------------------------------------------------------------------------------
// K1 with dense columns (tlpk_options.dense_cols): [A_s D_s A_s' + Rd, A_d; A_d', -(Theta_d^-1 + Rp_d)] of order m + k.  Its graph is
// that of B B' for the incidence matrix B (m + k rows) whose first n columns are A's with the dense ones emptied (constraint nodes: the
// pattern of A_s A_s') and whose further columns hold one entry A[i,j] of dense column j = dense[t] each: A[i,j] on row i, 1 on node m + t
// (the dense node is adjacent to the rows of its column, no clique).  The dense nodes go last (general path: behind the AMD order of the
// constraint nodes; block path: block -1, the root front), carry the sign -1 and are factorised by the signed instances of K2; step 14
// builds the assembly lists of this layout.  Afterwards S.Ap ... hold A itself: the solve, refinement and device-resident kernels read the
// caller's full A in K1 layout.
// ---------------------------------------------------------------------------------------------
int analyse_dense(Symbolic &S, i64 m, i64 n, const i64 *colptr, const i64 *rowval, const double *nzval,
                  int base, const Options &opt_in, const std::vector<i64> &dense) {
    if (m < 0 || n < 0 || (base != 0 && base != 1) || !colptr) return fail(S, TLPK_BADARG, "bad dimensions or index base");
    if (opt_in.nranks != 1) return fail(S, TLPK_BADARG, "dense_cols: one rank only");
    const i64 k = (i64)dense.size(), nnz = colptr[n] - base;
    if (nnz < 0 || m + k >= ((i64)1 << 31) || n >= ((i64)1 << 31) || nnz >= ((i64)1 << 30)) return fail(S, TLPK_TOO_LARGE, "m + dense columns or nnz(A) exceeds int32");
    if (nnz > 0 && (!rowval || !nzval)) return fail(S, TLPK_BADARG, "null rowval/nzval");
    for (i64 j = 0; j < n; ++j)
        if (colptr[j] - base < 0 || colptr[j + 1] < colptr[j] || colptr[j + 1] - base > nnz) return fail(S, TLPK_BADARG, "colptr not monotone");
    std::vector<char> isd((size_t)n, 0);
    i64 nnz_d = 0;
    for (i64 t = 0; t < k; ++t) {
        const i64 j = dense[(size_t)t];
        if (j < 0 || j >= n || (t > 0 && j <= dense[(size_t)t - 1])) return fail(S, TLPK_INTERNAL, "dense columns not ascending");
        isd[(size_t)j] = 1; nnz_d += colptr[j + 1] - colptr[j];
    }
    const i64 nb = n + nnz_d;
    if (nb >= ((i64)1 << 31)) return fail(S, TLPK_TOO_LARGE, "incidence matrix exceeds int32");
    std::vector<i64> bp((size_t)nb + 1), bi; std::vector<double> bx;
    bi.reserve((size_t)(nnz + nnz_d)); bx.reserve((size_t)(nnz + nnz_d));
    for (i64 j = 0; j < n; ++j) {
        bp[(size_t)j] = (i64)bi.size();
        if (isd[(size_t)j]) continue;
        for (i64 p = colptr[j] - base; p < colptr[j + 1] - base; ++p) {
            const i64 r = rowval[p] - base;
            if (r < 0 || r >= m) return fail(S, TLPK_BADARG, "row index out of range");
            bi.push_back(r); bx.push_back(nzval[p]);
        }
    }
    i64 col = n;
    for (i64 t = 0; t < k; ++t) {
        const i64 j = dense[(size_t)t];
        for (i64 p = colptr[j] - base; p < colptr[j + 1] - base; ++p) {
            const i64 r = rowval[p] - base;
            if (r < 0 || r >= m) return fail(S, TLPK_BADARG, "row index out of range");
            bp[(size_t)col++] = (i64)bi.size();
            bi.push_back(r); bx.push_back(nzval[p]);                 // constraint node
            bi.push_back(m + t); bx.push_back(1.0);                  // dense node
        }
    }
    bp[(size_t)nb] = (i64)bi.size();
    Options opt = opt_in;
    opt.system = 0; opt.n_dense = k;
    std::vector<i64> node_block;
    if (opt_in.row_block) {                    // the dense nodes join the linking rows in the root front
        node_block.assign((size_t)(m + k), -1);
        std::copy(opt_in.row_block, opt_in.row_block + m, node_block.begin());
        opt.row_block = node_block.data();
    }
    S.n_dense = k; S.dense_n = n; S.dense_cols = dense;
    int rc = analyse_common(S, m + k, nb, bp.data(), bi.data(), bx.data(), 0, opt);
    if (rc != TLPK_OK) return rc;
    S.csign.resize((size_t)(m + k));
    for (i64 kk = 0; kk < m + k; ++kk) S.csign[(size_t)kk] = (S.perm[(size_t)kk] >= m) ? -1.0 : 1.0;
    opt.row_block = nullptr;                    // (points into a local; analyse_rank reads the copy inside S)
    rc = analyse_rank(S, opt);
    if (rc != TLPK_OK) return rc;
    // the matrix kept for SpMV: A itself (CSC + CSR, the layout analyse_common builds for K1)
    S.n = n; S.nnzA = nnz;
    S.Ap.assign((size_t)n + 1, 0); S.Ai.resize((size_t)nnz); S.Ax.resize((size_t)nnz); S.Acol.resize((size_t)nnz);
    for (i64 j = 0; j < n; ++j) {
        S.Ap[(size_t)j + 1] = colptr[j + 1] - base;
        for (i64 p = colptr[j] - base; p < colptr[j + 1] - base; ++p) { S.Ai[(size_t)p] = (i32)(rowval[p] - base); S.Ax[(size_t)p] = nzval[p]; S.Acol[(size_t)p] = (i32)j; }
    }
    S.Tp.assign((size_t)m + 1, 0); S.Tj.resize((size_t)nnz); S.Tpos.resize((size_t)nnz);
    for (i64 p = 0; p < nnz; ++p) S.Tp[(size_t)S.Ai[(size_t)p] + 1]++;
    for (i64 i = 0; i < m; ++i) S.Tp[(size_t)i + 1] += S.Tp[(size_t)i];
    {
        std::vector<i64> cur(S.Tp.begin(), S.Tp.end() - 1);
        for (i64 p = 0; p < nnz; ++p) { const i64 q = cur[(size_t)S.Ai[(size_t)p]]++; S.Tj[(size_t)q] = S.Acol[(size_t)p]; S.Tpos[(size_t)q] = (i32)p; }
    }
    S.col_local.assign((size_t)n, 1);
    return TLPK_OK;
}

// ---------------------------------------------------------------------------------------------
// Dense constraint matrix (tlpk_create_dense; the reference's dense backend, src/KKT/Dense/lapack.jl:52-119).  A matrix without zeros
// gives a full S = A D A' + Rd: identity order (nothing to reduce), the elimination tree is the chain 0 -> 1 -> ... -> m - 1, column j
// of L has m - j entries, ONE supernode of m columns without children.  Written down directly -- steps 1 - 9 and 13 - 14 of the sparse
// analysis would spend n m (m + 1) / 2 list entries to find the same --, then the storage offsets of step 12 and the schedules of
// build_schedule for that front.  S itself is formed by k_dense_syrk (dense_kernels.hip) straight into the packed panel.
// ---------------------------------------------------------------------------------------------
int analyse_dense_matrix(Symbolic &S, i64 m64, i64 n64) {
    if (m64 < 1 || n64 < 0) return fail(S, TLPK_BADARG, "dense matrix: m >= 1, n >= 0");
    if (m64 >= ((i64)1 << 24) || n64 >= ((i64)1 << 31)) return fail(S, TLPK_TOO_LARGE, "dense matrix: m < 2^24 and n < 2^31");
    const i32 m = (i32)m64;
    S.m = m64; S.n = n64; S.nnzA = m64 * n64; S.system = 0; S.dense_matrix = 1;
    S.perm.resize((size_t)m); S.iperm.resize((size_t)m); S.parent.resize((size_t)m); S.colcount.resize((size_t)m); S.sn_of_col.assign((size_t)m, 0);
    S.flops_chol = 0;
    for (i32 j = 0; j < m; ++j) {
        S.perm[(size_t)j] = S.iperm[(size_t)j] = j;
        S.parent[(size_t)j] = (j + 1 < m) ? j + 1 : -1;
        S.colcount[(size_t)j] = m - j;
        S.flops_chol += (double)(m - j) * (double)(m - j);
    }
    S.Sp.assign((size_t)m + 1, 0);                 // no pattern of S is stored: every column "holds" no listed entry
    S.nnzS = S.nnzL = m64 * (m64 + 1) / 2;
    S.flops_syrk = (double)n64 * (double)m64 * (double)(m64 + 1);
    S.nsuper = 1; S.max_front = m; S.nblocks = 0; S.root_front = -1; S.ngroups = 1; S.n_local_blocks = 0;
    FrontDesc w{};
    w.f = m; w.ns = m; w.col0 = 0; w.parent = -1; w.child_ptr = 0; w.nchild = 0; w.rowoff = 0; w.reloff = 0; w.eatab = -1; w.flagoff = -1; w.ubuf = 0;
    w.lda = (w.f >= LDA_PAD_MIN_F) ? (w.f + 15) / 16 * 16 : w.f;                      // step 12
    w.loff = 0; S.lval_len = pk_len(w.lda, w.ns);
    w.uoff = 0; w.ucoff = 0; S.uc_len = 0; S.ubuf_len[0] = S.ubuf_len[1] = 0;
    w.dinvoff = 0; S.dinv_len = (w.ns >= NB_IN) ? (i64)((w.ns + NB_IN - 1) / NB_IN) * NB_IN * NB_IN : (i64)w.ns * w.ns;
    S.fronts.assign(1, w);
    S.rowidx.resize((size_t)m);
    for (i32 j = 0; j < m; ++j) S.rowidx[(size_t)j] = j;
    S.sparent_v.assign(1, -1);
    S.depth.assign(1, 0); S.nlevels = 1; S.level_ptr = {0, 1}; S.level_fronts.assign(1, 0);
    S.front_block.assign(1, -1); S.front_local.assign(1, 1); S.front_group.assign(1, 0); S.front_fa.assign(1, 0);
    S.col_local.assign((size_t)n64, 1); S.row_local.assign((size_t)m, 1);
    S.skip_off.assign(1, -1);                      // no amalgamation padding: nothing to skip
    S.gth_ptr.assign((size_t)m + 1, 0);            // no children: empty gather lists
    {
        const double f = m;
        S.flops_panel = f * f * f / 3.0;
        S.flops_update_alg = 0;
        for (i32 c = 0; c < m; ++c) { const double l = (double)(m - c) - (double)(std::min((c / NB_OUT + 1) * NB_OUT, m) - c); if (l > 0) S.flops_update_alg += l * l; }
    }
    S.error.clear();
    build_schedule(S);
    if (!S.error.empty()) return TLPK_INTERNAL;
    for (const UpdateTask &u : S.update_tasks)
        if ((u.k0 & 15) != 0) return fail(S, TLPK_INTERNAL, "update task: K range does not start on a multiple of 16 columns");
    S.zero_tasks.clear(); S.zero_small.clear(); S.n_zero_lower = 0;      // k_dense_syrk writes every stored entry of the panel: no zero-fill
    // k_dense_syrk: 128 x 128 tiles of the lower triangle, two workgroups per CU = 512 at a time.  When the tiles do not fill whole rounds of 512
    // (m = 2048: 136 tiles; m = 4096: 528 tiles = one full round and 16 stragglers) K = n is cut into parts of whole 16-column slabs, one workgroup
    // each, whose raw tiles k_dense_syrk_reduce sums in part order: the smallest number of parts that fills its rounds best (2 % or more over
    // every smaller one), with at least 512 columns per part (a part writes a 128 KB raw tile; 64 while the first round is not full) and at most
    // 4096 raw tiles of scratch.
    const i64 T = (m64 + TILE - 1) / TILE, ntiles = T * (T + 1) / 2;
    i64 split = 1;
    {
        auto fill = [&](i64 s_) { const i64 w_ = ntiles * s_; return (double)w_ / (double)((w_ + 511) / 512 * 512); };
        double best = fill(1);
        for (i64 s_ = 2; s_ <= 64 && ntiles * s_ <= 4096; ++s_) {
            if (n64 / s_ < (ntiles * s_ <= 512 ? 64 : 512)) break;            // (inside the first round -- small m -- shorter parts still pay)
            if (fill(s_) >= best + 0.02) { best = fill(s_); split = s_; }
        }
    }
    const i64 kc = std::max<i64>(16, ((n64 + split - 1) / split + 15) / 16 * 16);
    split = std::max<i64>(1, (n64 + kc - 1) / kc);
    S.syrk_split = (i32)split; S.syrk_kc = kc;
    S.syrk_slots = split > 1 ? ntiles * split : 0;
    S.spart_len = std::max(S.spart_len, S.syrk_slots * TILE * TILE);      // (shared with k_update's split-K parts: the product is complete before the factorisation starts)
    // k_dense_gemv_n: row blocks x column chunks, ~1024 workgroups
    const i64 rowblocks = (dense_lda(m64) + DGEMV_ROWS - 1) / DGEMV_ROWS;
    i64 chunks = std::max<i64>(1, std::min<i64>(1024 / rowblocks, (n64 + 15) / 16));
    const i64 cw = std::max<i64>(1, (n64 + chunks - 1) / chunks);
    S.gemv_chunks = std::max<i64>(1, (n64 + cw - 1) / cw);
    S.gemv_cw = std::max<i64>(1, (n64 + S.gemv_chunks - 1) / S.gemv_chunks);      // (what the kernels get: the width that spreads n over the chunks kept)
    return TLPK_OK;
}

// ---------------------------------------------------------------------------------------------
// New values on an analysed pattern (tlpk_set_values).  Nothing of the analysis depends on the values; what does is pair_w and the
// value arrays of A (Ax, the CSR copies Tx / Px).  build_value_maps re-walks the products of this rank's fronts with walk_pairs -- the
// traversal of step 14 -- and records, for product t of the lists, the positions of its two factors in the CALLER's nzval
// (VM_ONE: the unit entry of an incidence column of K2 / a dense column; (VM_MINUS, VM_ONE): the constant -1 of a diagonal), and for
// every entry of the value arrays the position it copies.  Built on the first tlpk_set_values of a handle, not at create.
// ---------------------------------------------------------------------------------------------
int build_value_maps(const Symbolic &S, i32 rank, ValueMaps &M) {
    if (S.dense_matrix) return TLPK_OK;
    const i32 m = (i32)S.m;
    const i64 np = S.pair_ptr.empty() ? 0 : S.pair_ptr[(size_t)S.nnzS];
    // the incidence matrix the lists were built on, with the caller's position of every value: K1 -- A itself; K2 -- the columns
    // (1 on the variable node, A[i,j] on the constraint node) S still holds; dense columns -- rebuilt as analyse_dense builds it
    std::vector<i64> bp, tp; std::vector<i32> bi, tj, tpos, src;
    const i64 *Ap = S.Ap.data(), *Tp = S.Tp.data(); const i32 *Ai = S.Ai.data(), *Tj = S.Tj.data(), *Tpos = S.Tpos.data();
    i32 dense_m = -1;
    try {
        if (S.system == 1) {
            src.resize(S.Ax.size());
            for (size_t q = 0; q < src.size(); ++q) src[q] = (q & 1) ? (i32)(q >> 1) : VM_ONE;
            M.ax_src = src;
        } else if (S.n_dense > 0) {
            const i64 n = S.n, k = S.n_dense, mu = S.m - S.n_dense;
            dense_m = (i32)mu;
            std::vector<char> isd((size_t)n, 0);
            for (i64 j : S.dense_cols) isd[(size_t)j] = 1;
            bp.reserve((size_t)n + 1);
            for (i64 j = 0; j < n; ++j) {
                bp.push_back((i64)bi.size());
                if (isd[(size_t)j]) continue;
                for (i64 p = S.Ap[(size_t)j]; p < S.Ap[(size_t)j + 1]; ++p) { bi.push_back(S.Ai[(size_t)p]); src.push_back((i32)p); }
            }
            for (i64 t = 0; t < k; ++t) {
                const i64 j = S.dense_cols[(size_t)t];
                for (i64 p = S.Ap[(size_t)j]; p < S.Ap[(size_t)j + 1]; ++p) {
                    bp.push_back((i64)bi.size());
                    bi.push_back(S.Ai[(size_t)p]); src.push_back((i32)p);          // constraint node
                    bi.push_back((i32)(mu + t)); src.push_back(VM_ONE);           // dense node
                }
            }
            bp.push_back((i64)bi.size());
            const i64 nb = (i64)bp.size() - 1, nz = (i64)bi.size();
            tp.assign((size_t)m + 1, 0); tj.resize((size_t)nz); tpos.resize((size_t)nz);
            for (i64 p = 0; p < nz; ++p) tp[(size_t)bi[(size_t)p] + 1]++;
            for (i32 i = 0; i < m; ++i) tp[(size_t)i + 1] += tp[(size_t)i];
            std::vector<i64> cur(tp.begin(), tp.end() - 1);
            for (i64 j = 0; j < nb; ++j)
                for (i64 p = bp[(size_t)j]; p < bp[(size_t)j + 1]; ++p) { const i64 q = cur[(size_t)bi[(size_t)p]]++; tj[(size_t)q] = (i32)j; tpos[(size_t)q] = (i32)p; }
            Ap = bp.data(); Ai = bi.data(); Tp = tp.data(); Tj = tj.data(); Tpos = tpos.data();
        }
        M.pair_a.resize((size_t)np); M.pair_b.resize((size_t)np);
        const PairWalk W{Ap, Ai, Tp, Tj, Tpos, S.perm.data(), S.iperm.data(), S.col_local.data(), S.system, S.k2_n, rank, dense_m, (i32)S.dense_n, S.dense_cols.data()};
        const i32 *sv = src.empty() ? nullptr : src.data();
        const unsigned nthreads = host_threads(S.nsuper);
        struct Scratch { std::vector<i64> cur; };
        std::vector<Scratch> sc(nthreads);
        std::atomic<int> bad{0};
        const bool ok = parallel_for(S.nsuper, nthreads, [&](unsigned tid, i64 s64) {
            const i32 s = (i32)s64;
            if (!S.front_local[(size_t)s]) return;
            const FrontDesc &w = S.fronts[(size_t)s];
            std::vector<i64> &cur = sc[tid].cur;                      // per permuted row: the next free slot of its entry in the current column
            if (cur.empty()) cur.assign((size_t)m, -1);
            const bool is_root = (s == S.root_front);
            for (i32 kk = w.col0; kk < w.col0 + w.ns; ++kk) {
                for (i64 e = S.Sp[(size_t)kk]; e < S.Sp[(size_t)kk + 1]; ++e) cur[(size_t)S.Si[(size_t)e]] = S.pair_ptr[(size_t)e];
                walk_pairs(W, kk, is_root, [&](i32 ii, i64 pa, i64 pb, i32) {
                    const i64 t = cur[(size_t)ii]++;
                    if (t < 0 || t >= np) { bad = 1; return; }
                    if (pa < 0) { M.pair_a[(size_t)t] = VM_MINUS; M.pair_b[(size_t)t] = VM_ONE; }
                    else { M.pair_a[(size_t)t] = sv ? sv[pa] : (i32)pa; M.pair_b[(size_t)t] = sv ? sv[pb] : (i32)pb; }
                });
                for (i64 e = S.Sp[(size_t)kk]; e < S.Sp[(size_t)kk + 1]; ++e)
                    if (cur[(size_t)S.Si[(size_t)e]] != S.pair_ptr[(size_t)e + 1]) bad = 1;       // the walk must fill every entry's range exactly
            }
        }, 64);
        if (!ok) return TLPK_OOM;
        if (bad) return TLPK_INTERNAL;
        // the CSR copies: Tx[q] = value[Tpos[q]]; Px = the same rows in permuted order (K1; tlpk_api.cpp: upload_all)
        M.tx_src.resize(S.Tpos.size());
        for (size_t q = 0; q < S.Tpos.size(); ++q) M.tx_src[q] = (S.system == 1) ? M.ax_src[(size_t)S.Tpos[q]] : S.Tpos[q];
        if (S.system == 0) {
            const i64 mu = S.m - S.n_dense;
            M.px_src.reserve(S.Tpos.size());
            for (i64 ii = 0; ii < S.m; ++ii) {
                const i32 i = S.perm[(size_t)ii];
                if (i >= mu) continue;
                for (i64 q = S.Tp[(size_t)i]; q < S.Tp[(size_t)i + 1]; ++q) M.px_src.push_back(S.Tpos[(size_t)q]);
            }
        }
    } catch (const std::bad_alloc &) { return TLPK_OOM; }
    M.built = true;
    return TLPK_OK;
}

// ---------------------------------------------------------------------------------------------
// Matrix-free handle (tlpk_options.krylov): the CSC copy of A and its row-wise copy in the caller's order, identity "permutation", and
// nothing else -- no ordering, no pattern of S, no fronts, lists or schedules.  Host time and memory O(nnz(A) + m + n).
// ---------------------------------------------------------------------------------------------
int analyse_krylov(Symbolic &S, i64 m, i64 n, const i64 *colptr, const i64 *rowval, const double *nzval, int base) {
    if (m < 0 || n < 0 || (base != 0 && base != 1) || !colptr) return fail(S, TLPK_BADARG, "bad dimensions or index base");
    if (m >= (i64)1 << 31 || n >= (i64)1 << 31) return fail(S, TLPK_TOO_LARGE, "m or n exceeds int32");
    const i64 nnz = colptr[n] - base;
    if (nnz < 0 || nnz >= (i64)1 << 31) return fail(S, TLPK_TOO_LARGE, "nnz(A) exceeds int32");
    if (nnz > 0 && (!rowval || !nzval)) return fail(S, TLPK_BADARG, "null rowval/nzval");
    S.m = m; S.n = n; S.nnzA = nnz; S.system = 0;
    S.Ap.resize((size_t)n + 1); S.Ai.resize((size_t)nnz); S.Ax.resize((size_t)nnz);
    S.Tp.assign((size_t)m + 1, 0); S.Tj.resize((size_t)nnz); S.Tpos.resize((size_t)nnz);
    for (i64 j = 0; j <= n; ++j) {
        S.Ap[(size_t)j] = colptr[j] - base;
        if (S.Ap[(size_t)j] < 0 || S.Ap[(size_t)j] > nnz || (j > 0 && S.Ap[(size_t)j] < S.Ap[(size_t)j - 1])) return fail(S, TLPK_BADARG, "colptr not monotone");
    }
    if (n > 0 && S.Ap[0] != 0) return fail(S, TLPK_BADARG, "colptr does not start at index_base");
    for (i64 p = 0; p < nnz; ++p) {
        const i64 r = rowval[p] - base;
        if (r < 0 || r >= m) return fail(S, TLPK_BADARG, "row index out of range");
        S.Ai[(size_t)p] = (i32)r; S.Ax[(size_t)p] = nzval[p];
        S.Tp[(size_t)r + 1]++;
    }
    for (i64 i = 0; i < m; ++i) S.Tp[(size_t)i + 1] += S.Tp[(size_t)i];
    {
        std::vector<i64> cur(S.Tp.begin(), S.Tp.end() - 1);
        for (i64 j = 0; j < n; ++j)
            for (i64 p = S.Ap[(size_t)j]; p < S.Ap[(size_t)j + 1]; ++p) {         // column order inside a row: the order the direct handles' row-wise copy has
                const i64 q = cur[(size_t)S.Ai[(size_t)p]]++;
                S.Tj[(size_t)q] = (i32)j; S.Tpos[(size_t)q] = (i32)p;
            }
    }
    S.perm.resize((size_t)m); S.iperm.resize((size_t)m);
    for (i64 i = 0; i < m; ++i) S.perm[(size_t)i] = S.iperm[(size_t)i] = (i32)i;
    S.row_local.assign((size_t)m, 1); S.col_local.assign((size_t)n, 1);
    S.pair_ptr.assign(1, 0);                       // (no entry of S, no product)
    S.nsuper = 0; S.nlevels = 0; S.nblocks = 0; S.root_front = -1; S.ngroups = 1; S.n_local_blocks = 0;
    S.error.clear();
    return TLPK_OK;
}

// the host side of a refresh: the value array of the analysed matrix and -- where the host still holds them (analyse-only handles) -- the products
void host_set_values(Symbolic &S, const ValueMaps &M, const double *nz) {
    if (S.system == 1) { for (size_t q = 1; q < S.Ax.size(); q += 2) S.Ax[q] = nz[q >> 1]; }
    else std::memcpy(S.Ax.data(), nz, S.Ax.size() * sizeof(double));
    if (S.pair_w.empty()) return;
    const i64 np = (i64)S.pair_w.size();
    constexpr i64 CH = (i64)1 << 16;
    const i64 nch = (np + CH - 1) / CH;
    auto val = [&](i32 p) { return p >= 0 ? nz[p] : (p == VM_ONE ? 1.0 : -1.0); };
    (void)parallel_for(nch, host_threads(nch), [&](unsigned, i64 ch) {
        for (i64 t = ch * CH, t1 = std::min(np, t + CH); t < t1; ++t) S.pair_w[(size_t)t] = val(M.pair_a[(size_t)t]) * val(M.pair_b[(size_t)t]);
    });
}

}  // namespace tlpk
