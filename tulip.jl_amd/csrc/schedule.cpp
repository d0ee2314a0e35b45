// schedule.cpp -- launch schedules of the analyse phase.  All task lists are static for the lifetime of the handle: one IPM run
// replays them once per update! (factor) and 2..6 times per Newton step (solves).
// build_schedule (at the end of this file) drives a ScheduleBuilder: singles and upper fronts, zero-fill lists; per stream group and level the
// factorisation (front assembly, extend-add, the blocked partial factorisation as launches or as one LK_CHAIN launch, extend-add of U); absolute
// split-K slots; the flags of the sweeps; the forward and the backward solve.  What a piece depends on is in its signature: the level's plan
// (LevelPlan), the stream a launch goes to (Scope), the pass over the level's fronts (Pass), where tiles go (TileSink).  Every environment setting
// is read in read_knobs.
#include "schedule.hpp"

#include <climits>
#include <map>
#include <numeric>
#include <unordered_map>
#include <utility>

namespace tlpk {
namespace {

// ---------------------------------------------------------------------------------------------
// Every environment setting the schedule reads.  Lifetime P: read by the first analysis of the process and fixed from then on;
// lifetime A: read again by every analysis (build_schedule call).  Experiments and diagnostics keep their measurements where they act.
//   name                    default  life  meaning
//   TLPK_DEFER_UPPER        1        P     zero-fill + assembly of the upper fronts on a stream of their own (0 = one-stream order)
//   TLPK_SKIP_WIN           128      P     rows a skip decision looks at: 128 | 256 | 512 (anything else = 128)
//   TLPK_EA_BANDS           1        P     row bands per extend-add column range of the parents with f >= 2048 (>= 1)
//   TLPK_UPD_LPT            0        P     1 = the tiles of an update launch longest first
//   TLPK_UPD_SUPER          4        A     super-tile edge of the update tile order, in tiles (>= 1)
//   TLPK_CHAIN_TILE64       2        A     diagonal block's short update in a chain: 0 = 128 x 128 tiles, 1 = 64 x 64, other = 32 x 32
//   TLPK_LOOKAHEAD          auto     A     look-ahead for the diagonal blocks: 0 = off, other = on, unset = by the level's big fronts
//   TLPK_TAIL_SLOTS         0        A     tail split of an update launch on this many slots (0 = off)
//   TLPK_TAIL64             0        A     last round of an update launch as 64 x 64 tiles when it holds at most this many tiles (0 = off)
//   TLPK_TAIL64_SLOTS       512      A     resident 128 x 128 tiles the tail shape assumes (>= 1; for the CPU tests on small LPs)
//   TLPK_KSPLIT_LEN         0        A     look-ahead levels: longest K range of one update item (0 = off)
//   TLPK_SPLITK_TILES       256      A     split-K when a launch has fewer tiles than this / 2 (0 = off)
//   TLPK_MACRO_TILES        2048     A     tiles wanted in a macro column's long-K launch (0 = no macro columns)
//   TLPK_LA_FULL            0        A     1 = every block column of a look-ahead level pulls its long K one block column early
//   TLPK_LA_MACRO           1        A     0 = no macro columns on the look-ahead levels
//   TLPK_CHAIN              auto     A     LK_CHAIN: 0 = off, > 0 = every level with a multi-block-column front, unset / < 0 = by the rule
//   TLPK_CHAIN_MAX_FRONTS   8        A     the rule: at most this many multi-block-column fronts on the level (>= 1)
//   TLPK_CHAIN_MIN_NS       769      A     the rule: the widest of them has at least this many pivot columns
//   TLPK_CHAIN_JIT          0        A     1 = macro-column tiles take their tickets just in time
//   TLPK_CHAIN_EARLY        1        A     0 = the strips of a full-width block column wait for its complete diagonal block
//   TLPK_POTRF_MODE, _WAVE, _PAIR, _DYN   A     (kernels' knobs) a non-default diagonal-block kernel keeps the launches: no LK_CHAIN
//   TLPK_SWEEP              1        A     0 = one launch per 128-column block step instead of the persistent sweeps
//   TLPK_SOLVE_MERGE        256      A     small fronts ride in a sweep of at most this many items (0 = never)
//   TLPK_SOLVE_SIDE         0        A     1 = the small fronts of a level on the side stream beside its sweep
//   TLPK_SOLVE_ONE_GROUP    1        A     0 = one solve schedule per stream group
// ---------------------------------------------------------------------------------------------
struct ScheduleKnobs {
    bool defer_upper; i32 skip_win; i32 ea_bands; bool upd_lpt;                       // lifetime P
    i32 upd_super; i32 chain_tile; int lookahead; i64 tail_slots, tail64, tail64_slots; i32 ksplit_len; i64 splitk_tiles, macro_tiles; bool la_full, la_macro;
    int chain; i32 chain_max_fronts, chain_min_ns; bool chain_jit, chain_early, potrf_default;
    bool sweep; i64 solve_merge; bool solve_side, solve_one_group;
};
ScheduleKnobs read_knobs() {
    static const bool defer_upper = [] { const char *e = std::getenv("TLPK_DEFER_UPPER"); return !e || std::atoi(e) != 0; }();
    static const i32 skip_win = [] { const char *e = std::getenv("TLPK_SKIP_WIN"); const int v = e ? std::atoi(e) : TILE; return (v == 256 || v == 512) ? v : TILE; }();
    static const i32 ea_bands = [] { const char *e = std::getenv("TLPK_EA_BANDS"); return e ? std::max(1, std::atoi(e)) : 1; }();
    static const bool upd_lpt = [] { const char *e = std::getenv("TLPK_UPD_LPT"); return e && std::atoi(e) != 0; }();
    auto num = [](const char *name, int dflt) { const char *e = std::getenv(name); return e ? std::atoi(e) : dflt; };
    auto num64 = [](const char *name, i64 dflt) { const char *e = std::getenv(name); return e ? (i64)std::atoll(e) : dflt; };
    auto on = [](const char *name) { const char *e = std::getenv(name); return e && std::atoi(e) != 0; };           // default off
    auto not_off = [](const char *name) { const char *e = std::getenv(name); return !e || std::atoi(e) != 0; };     // default on
    ScheduleKnobs K{};
    K.defer_upper = defer_upper; K.skip_win = skip_win; K.ea_bands = ea_bands; K.upd_lpt = upd_lpt;
    K.upd_super = std::max(1, num("TLPK_UPD_SUPER", 4));
    K.chain_tile = [&] { const int v = num("TLPK_CHAIN_TILE64", 2); return v == 0 ? TILE : (v == 1 ? 64 : 32); }();
    K.lookahead = [] { const char *e = std::getenv("TLPK_LOOKAHEAD"); return e ? (std::atoi(e) != 0 ? 1 : 0) : -1; }();
    K.tail_slots = num64("TLPK_TAIL_SLOTS", 0);
    K.tail64 = std::max(0, num("TLPK_TAIL64", 0)); K.tail64_slots = std::max(1, num("TLPK_TAIL64_SLOTS", 512));
    K.ksplit_len = std::max(0, num("TLPK_KSPLIT_LEN", 0));       // (multiples of 16 keep the parts on slab boundaries)
    K.splitk_tiles = num64("TLPK_SPLITK_TILES", 256); K.macro_tiles = num64("TLPK_MACRO_TILES", 2048);
    K.la_full = on("TLPK_LA_FULL"); K.la_macro = not_off("TLPK_LA_MACRO");
    K.chain = num("TLPK_CHAIN", -1); K.chain_max_fronts = std::max(1, num("TLPK_CHAIN_MAX_FRONTS", 8)); K.chain_min_ns = num("TLPK_CHAIN_MIN_NS", 769);
    K.chain_jit = on("TLPK_CHAIN_JIT"); K.chain_early = not_off("TLPK_CHAIN_EARLY");
    K.potrf_default = [] {
        const char *m = std::getenv("TLPK_POTRF_MODE");
        return (!m || (std::atoi(m) & 3) == 3) && !std::getenv("TLPK_POTRF_WAVE") && !std::getenv("TLPK_POTRF_PAIR") && !std::getenv("TLPK_POTRF_DYN");
    }();
    K.sweep = not_off("TLPK_SWEEP");
    K.solve_merge = std::max(0, num("TLPK_SOLVE_MERGE", 256));
    K.solve_side = on("TLPK_SOLVE_SIDE"); K.solve_one_group = not_off("TLPK_SOLVE_ONE_GROUP");
    return K;
}

// The stream a launch belongs to: stream group `group` (fronts at depth >= 1 of that group) or -1 = the depth-0 fronts, which run on the main
// stream after all groups joined; side = 1: the group's side stream.
struct Scope { int group, side; };
// Round 6: the fronts of the level with more than one block column may run as ONE dependency-driven launch (LK_CHAIN, below): PASS_ALL = every front
// through the launches; PASS_LAUNCH = the other fronts through the launches, PASS_CHAIN = the chain fronts, their launches CAPTURED and turned into items.
// The decisions that look at the whole level (split-K, macro columns, look-ahead) see all of the rank's fronts in every pass: a tile is the same
// tile whichever way it is launched.
enum Pass : int { PASS_ALL = 0, PASS_LAUNCH = 1, PASS_CHAIN = 2 };
struct Cap { i32 kind; i64 first, count; };               // a captured launch
// Where push_update_region puts its tiles.  count != nullptr: a dry run that only counts them (into *count), for every front the caller passes;
// skip: tiles take skip lists (off for split-K launches: few tiles, the parts are cut by K position); chain: the tiles run inside k_chain.
struct TileSink { i64 *count; bool skip, chain; };
// One level of one stream group while its factorisation is scheduled.
struct LevelPlan {
    int g; i32 t0, t1;                               // scope and level_fronts range
    i32 max_ns = 0, nouter = 0;                      // widest pivot block of the scope's fronts; its block columns
    bool lookahead = false;
    std::vector<i32> mac_first, mac_G;               // macro column of every block column: block columns [mac_first[io], mac_first[io] + mac_G[io])
    std::vector<char> chain_front;                   // (only the entries of this level's fronts are ever set)
    // Canonical index of a tile inside its launch: position in the list that ALL of this rank's fronts of the level would
    // produce (level order), whatever the stream group the front runs in -- what the tail split is decided on.
    std::vector<i64> canon_count, canon_next;
    std::vector<i64> task_canon;                     // canonical index of every task pushed by the current launch
    std::vector<Cap> cap;                            // PASS_CHAIN: the captured launches
    i64 chain_slot_base = 0;                         // split-K scratch slots of a chain launch are never reused inside the launch
    i32 k_first(i32 io) const { return (io == mac_first[(size_t)io]) ? 0 : mac_first[(size_t)io] * NB_OUT; }   // block column io still needs K = [k_first, ko)
};

// entries of a tile that are targets: row >= column, row < f, column < c1
double tile_entries(const FrontDesc &w, i32 i0, i32 j0, i32 c1, i32 ts) {
    double e = 0;
    const i32 r1 = std::min(i0 + ts, w.f);
    for (i32 col = j0; col < std::min(j0 + ts, c1); ++col) e += std::max(0, r1 - std::max(i0, col));
    return e;
}

// ---- round 6: the dependency-driven form (LK_CHAIN) --------------------------------------------------------------------------------
// The launches of a block column -- diagonal tiles -> diagonal block -> rows-below tiles -> triangular solve, with their stream forks and joins --
// are a lock-step over ALL fronts of the level and four or five launch gaps per 256 columns; where a level has few fronts (a pds-class top front,
// the root front, the blocks of one rank of an 8-GPU job) the chain potrf(io) -> trsm(io) -> diagonal update(io + 1) IS the level's time, and
// profiles/r05_chain_overlap.txt showed that it never runs beside the rows-below tiles it was forked to hide behind.  Here the SAME tasks (same
// tiles, same K ranges, same split-K parts: the captured launches of PASS_CHAIN) become the items of one persistent launch: a workgroup draws an
// item, waits for the completion counters the item names, runs the task's ordinary device function and publishes its stores with one agent-scope
// release before it raises its counter (cdna_hip_programming.md, Guideline 16, counter form).  Ticket order = the order of the captured launches
// = block column major: diagonal tiles, diagonal block, rows-below tiles (+ look-ahead / macro-column tiles), strips of the triangular solve.
// Every wait names counters raised by EARLIER items only, so no schedule of the workgroups can deadlock (tests/emulate.py asserts it).
// Adders of one target tile (macro-column tile, look-ahead tile, the block column's own tile or its split-K reduction) are chained through the
// tile's counter in that order: exactly the order of the launches, so the factor is bit-identical to the launch form (TLPK_CHAIN=0).
struct ChainBuilder {
    struct FC { i64 base; i32 nbc, ntr, nsl, stride; };         // counters of one front: `stride` per block column, from local counter `base`
    struct Unit { i64 first, count, red; };                    // update tasks [first, first + count) (one tile: itself, or its split-K parts) and its reduce task (or -1)
    Symbolic &S;
    // jit (TLPK_CHAIN_JIT=1; default off): the macro-column tiles take their tickets just in time, see `held` below; off = in the order of the launches.
    // early (TLPK_CHAIN_EARLY, default 1): the strips of a full-width block column do not wait for its diagonal block to be complete -- the diagonal-block role
    // raises the block column's counter on its way (+1 behind each of its first three 64-wide steps, its final signal makes 4) and the strip role waits for
    // the value each of its ten operand blocks needs (kernels.hip: trsm_task_dma).  Here: the strip's item drops the wait (w2), its task names the
    // counter (pad2 = global index + 1), the diagonal block's item is marked (sub = 1).  Same tickets, same data flow, same bits.
    const bool jit, early;
    std::unordered_map<i32, FC> fc;
    i64 cbase = 0;                                               // global index of local counter q: cbase + q
    std::vector<i32> expect;                                     // signals handed out so far, per local counter
    std::unordered_map<i64, char> covered;                       // target tiles of a diagonal block that a 64 x 64 tile waits for (the diagonal block then needs not)
    // Tickets are priorities, and a workgroup keeps the item it drew: at the start of a macro column the launch order puts ~900 tiles with K = [0, kM) --
    // the long update of the macro column's OTHER block columns, hundreds of microseconds each even cut by K length -- in front of the chain's next links,
    // which then wait for a free workgroup (profiles/r06_chain_trace_pds*.txt: 0.3 - 0.7 ms stalls at every macro column start; putting them all behind
    // the strips of that block column, round 6's first try, only moved the stall to the next block column).  Just in time: the tiles that feed block
    // column io_t are held back until block column io_t - 2 -- they take their tickets behind its rows-below tiles and in front of its strips, two links
    // of the chain before they are needed, one block column's worth at a time.  A held tile travels with its split-K parts and its reduction.  Every
    // adder of a target tile is still created before the later adders of that tile (the look-ahead tiles of block column io_t come with io_t - 1, its
    // own tiles with io_t): same order of the sums, same bits as the launch form.
    std::map<i32, std::vector<Unit>> held;                       // target block column -> units
    std::unordered_map<i32, i64> slot_red;                       // split-K scratch slot -> the counter of the reduction that owns it (slots are unique inside a chain launch)
    std::unordered_map<i64, i64> red_rc;                         // reduce task -> its counter
    i32 io_cur = -1;                                             // block column of the last diagonal block seen
    bool bad = false;

    ChainBuilder(Symbolic &S_, bool jit_, bool early_) : S(S_), jit(jit_), early(early_) {}
    i64 new_counter() { expect.push_back(0); return (i64)expect.size() - 1; }
    static i64 c_dg(const FC &c, i32 io, i32 pos) { return c.base + (i64)io * c.stride + pos; }                  // diagonal block of io: tiles (ko, ko) | (ko + 128, ko) | (ko + 128, ko + 128)
    static i64 c_pf(const FC &c, i32 io) { return c.base + (i64)io * c.stride + 3; }                             // the diagonal block is factored
    static i64 c_dq(const FC &c, i32 io) { return c.base + (i64)io * c.stride + 4; }                             // the 64 x 64 tiles of the diagonal block's last (short) update
    static i64 c_tg(const FC &c, i32 io, i32 tr, i32 cj) { return c.base + (i64)io * c.stride + 5 + 2 * tr + cj; }     // target tile (rows 128 tr .., column tile cj of block column io)
    static i64 c_ts(const FC &c, i32 io, i32 sl) { return c.base + (i64)io * c.stride + 5 + 2 * c.ntr + sl; }    // rows [64 sl, 64 sl + 64) are solved in block column io
    i32 G(i64 q) const { return (i32)(cbase + q); }
    // the counter an adder of target tile (i0, j0) raises, or -1 (targets in the update matrix: read by the next level's extend-add launch)
    static i64 target_counter(const FC &c, const FrontDesc &w, i32 i0, i32 j0) {
        if (j0 >= w.ns) return -1;
        const i32 io = j0 / NB_OUT, ko = io * NB_OUT;
        if (i0 < ko + NB_OUT) return c_dg(c, io, (i0 == ko) ? 0 : 1 + (j0 - ko) / TILE);
        return c_tg(c, io, i0 / TILE, (j0 - ko) / TILE);
    }
    // operand rows [r0, r0 + 128) of an update tile whose K range ends in block column io_k: hand-over flags of the strips that solved them
    void operand_wait(const FC &c, const FrontDesc &w, i32 io_k, i32 r0, i32 &wq, i32 &nq) {
        const i32 s0 = r0 / 64, s1 = (std::min(r0 + TILE, w.f) - 1) / 64;
        for (i32 sl = s0; sl <= s1; ++sl) if (expect[(size_t)c_ts(c, io_k, sl)] != 1) bad = true;      // no strip (or two) for these rows: a bug
        wq = G(c_ts(c, io_k, s0)); nq = s1 - s0 + 1;
    }
    void update_item(i64 q) {
        const UpdateTask &u = S.update_tasks[(size_t)q];
        const FrontDesc &w = S.fronts[u.front];
        const FC &c = fc.at(u.front);
        ChainItem it{CR_UPDATE, (i32)q, 0, 0, 0, 0, 0, 0, 0, -1, 0, -1};
        const i32 io_k = (u.k0 + u.kw - 1) / NB_OUT;
        operand_wait(c, w, io_k, u.i0, it.w0, it.n0); it.need0 = 1;
        if (u.j0 != u.i0) { operand_wait(c, w, io_k, u.j0, it.w1, it.n1); it.need1 = 1; }
        if (u.pad1) {
            const auto f = slot_red.find(u.pad1 - 1);
            if (f == slot_red.end()) { bad = true; return; }
            it.sig = G(f->second); ++expect[(size_t)f->second];
        } else if (u.pad2) {
            // a 64 x 64 tile of the diagonal block: ordered behind the earlier adders of the 128 x 128 target tile that holds it (look-ahead / macro-column
            // tiles) through that tile's counter, which it does NOT raise -- its siblings must not wait for it --; all of them raise one counter of their own
            const i32 io = u.j0 / NB_OUT, ko = io * NB_OUT;
            const i64 tc = target_counter(c, w, ko + ((u.i0 - ko) & ~(TILE - 1)), ko + ((u.j0 - ko) & ~(TILE - 1)));
            if (u.j0 >= w.ns || tc < 0 || u.i0 >= ko + NB_OUT) { bad = true; return; }
            if (expect[(size_t)tc] > 0) { it.w2 = G(tc); it.need2 = expect[(size_t)tc]; }
            covered[tc] = 1;
            it.sig = G(c_dq(c, io)); ++expect[(size_t)c_dq(c, io)];
        } else {
            const i64 tc = target_counter(c, w, u.i0, u.j0);
            if (tc >= 0) {
                if (expect[(size_t)tc] > 0) { it.w2 = G(tc); it.need2 = expect[(size_t)tc]; }     // the earlier adder(s) of this tile
                it.sig = G(tc); ++expect[(size_t)tc];
            }
        }
        S.chain_items.push_back(it);
    }
    void reduce_items(i64 q) {
        const UpdateTask &r = S.reduce_tasks[(size_t)q];
        const FrontDesc &w = S.fronts[r.front];
        const FC &c = fc.at(r.front);
        const i64 rc = red_rc.at(q);
        if (expect[(size_t)rc] != r.kw) { bad = true; return; }
        const i64 tc = target_counter(c, w, r.i0, r.j0);
        for (i32 sub = 0; sub < RED_SPLIT; ++sub) {
            ChainItem it{CR_REDUCE, (i32)q, sub, G(rc), 1, r.kw, 0, 0, 0, -1, 0, -1};
            if (tc >= 0) {
                if (expect[(size_t)tc] > 0) { it.w2 = G(tc); it.need2 = expect[(size_t)tc]; }
                it.sig = G(tc);
            }
            S.chain_items.push_back(it);
        }
        if (tc >= 0) expect[(size_t)tc] += RED_SPLIT;
    }
    void emit_units(const std::vector<Unit> &us) {           // the tiles first, then their reductions (the order of a launch pair)
        for (const Unit &u : us) for (i64 q = u.first; q < u.first + u.count && !bad; ++q) update_item(q);
        for (const Unit &u : us) if (u.red >= 0 && !bad) reduce_items(u.red);
    }
    void flush_held(i32 io_upto) {                           // the held tiles of the block columns <= io_upto, in block-column order
        while (!held.empty() && held.begin()->first <= io_upto && !bad) { emit_units(held.begin()->second); held.erase(held.begin()); }
    }
    // a captured update launch L and, if R != nullptr, the reduce launch behind it
    void update_launch_items(const Cap &L, const Cap *R) {
        // split-K parts of this launch: scratch slot -> the counter of the reduction that owns it
        std::unordered_map<i32, i64> slot_task;                // slot -> reduce task
        if (R)
            for (i64 q = R->first; q < R->first + R->count; ++q) {
                const UpdateTask &r = S.reduce_tasks[(size_t)q];
                const i64 rc = new_counter();
                red_rc[q] = rc;
                for (i32 sp = 0; sp < r.kw; ++sp) { slot_red[r.k0 + sp] = rc; slot_task[r.k0 + sp] = q; }
            }
        std::vector<Unit> now;
        i64 nred_seen = 0;
        for (i64 q = L.first; q < L.first + L.count && !bad;) {
            const UpdateTask &u = S.update_tasks[(size_t)q];
            Unit un{q, 1, -1};
            if (u.pad1) {                                    // the consecutive parts of one tile
                const auto f = slot_task.find(u.pad1 - 1);
                if (f == slot_task.end()) { bad = true; break; }
                un.red = f->second; ++nred_seen;
                while (q + un.count < L.first + L.count) {
                    const UpdateTask &v = S.update_tasks[(size_t)(q + un.count)];
                    const auto g = v.pad1 ? slot_task.find(v.pad1 - 1) : slot_task.end();
                    if (g == slot_task.end() || g->second != un.red) break;
                    ++un.count;
                }
            }
            const i32 io_t = (u.j0 < S.fronts[u.front].ns) ? u.j0 / NB_OUT : -1;
            if (jit && io_cur >= 0 && io_t >= io_cur + 3) held[io_t].push_back(un); else now.push_back(un);
            q += un.count;
        }
        if (R && nred_seen != R->count) bad = true;          // every reduction belongs to exactly one tile of this launch
        emit_units(now);
    }
    void potrf_items(const Cap &L) {
        for (i64 q = L.first; q < L.first + L.count; ++q) {
            const PotrfTask &pt = S.potrf_tasks[(size_t)q];
            io_cur = std::max(io_cur, pt.k0 / NB_OUT);
            const FC &c = fc.at(pt.front);
            const i32 io = pt.k0 / NB_OUT;
            ChainItem it{CR_POTRF, (i32)q, (early && pt.nb == NB_OUT) ? 1 : 0, 0, 0, 0, 0, 0, 0, -1, 0, G(c_pf(c, io))};
            // waits: the counter of the block's 64 x 64 tiles (they waited for the adders of their target tiles themselves), and every target tile
            // with adders that no 64 x 64 tile stands behind -- at most three counters in all
            i64 wl[4]; int nw = 0;
            if (expect[(size_t)c_dq(c, io)] > 0) wl[nw++] = c_dq(c, io);
            for (int pos = 0; pos < 3; ++pos) { const i64 d = c_dg(c, io, pos); if (expect[(size_t)d] > 0 && !covered.count(d)) wl[nw++] = d; }
            if (nw > 3) { bad = true; break; }
            if (nw > 0) { it.w0 = G(wl[0]); it.n0 = 1; it.need0 = expect[(size_t)wl[0]]; }
            if (nw > 1) { it.w1 = G(wl[1]); it.n1 = 1; it.need1 = expect[(size_t)wl[1]]; }
            if (nw > 2) { it.w2 = G(wl[2]); it.need2 = expect[(size_t)wl[2]]; }
            ++expect[(size_t)c_pf(c, io)];
            S.chain_items.push_back(it);
        }
    }
    void trsm_items(const Cap &L) {
        flush_held(io_cur + 2);                              // just in time: behind this block column's rows-below tiles, in front of its strips
        for (i64 q = L.first; q < L.first + L.count; ++q) {
            const TrsmTask &tt = S.trsm_tasks[(size_t)q];
            const FC &c = fc.at(tt.front);
            const i32 io = tt.k0 / NB_OUT, tr = tt.row0 / TILE;
            if (expect[(size_t)c_pf(c, io)] != 1 || tt.pad1 > (tt.row0 / 64 + 1) * 64) { bad = true; break; }
            ChainItem it{CR_TRSM, (i32)q, 0, 0, 0, 0, 0, 0, 0, G(c_pf(c, io)), 1, G(c_ts(c, io, tt.row0 / 64))};
            if (tr * TILE >= tt.k0 + NB_OUT) {              // (a strip inside the diagonal tiles' rows -- a narrow last block column -- is released by the diagonal block alone)
                const i64 g0 = c_tg(c, io, tr, 0), g1 = c_tg(c, io, tr, 1);
                if (expect[(size_t)g0] > 0) { it.w0 = G(g0); it.n0 = 1; it.need0 = expect[(size_t)g0]; }
                if (expect[(size_t)g1] > 0) { it.w1 = G(g1); it.n1 = 1; it.need1 = expect[(size_t)g1]; }
            }
            if (early && tt.nb == NB_OUT) { it.w2 = -1; it.need2 = 0; S.trsm_tasks[(size_t)q].pad2 = G(c_pf(c, io)) + 1; }
            ++expect[(size_t)c_ts(c, io, tt.row0 / 64)];
            S.chain_items.push_back(it);
        }
    }
    // the captured launches in order, then: the values the diagonal blocks and the strips wait for must be FINAL (nothing after them may add to their tiles)
    void run(const std::vector<Cap> &cap, i64 first_item) {
        for (size_t ci = 0; ci < cap.size() && !bad; ++ci) {
            const Cap &L = cap[ci];
            if (L.kind == LK_UPDATE) {
                const bool has_red = ci + 1 < cap.size() && cap[ci + 1].kind == LK_UPDATE_REDUCE;
                update_launch_items(L, has_red ? &cap[ci + 1] : nullptr);
                if (has_red) ++ci;                                   // the reduce launch is consumed
            } else if (L.kind == LK_POTRF || L.kind == LK_POTRF_WIDE) potrf_items(L);
            else if (L.kind == LK_TRSM) trsm_items(L);
            else bad = true;                                         // (no other kind is ever captured)
        }
        flush_held(INT32_MAX);
        for (i64 q = first_item; q < (i64)S.chain_items.size() && !bad; ++q) {
            const ChainItem &it = S.chain_items[(size_t)q];
            if (it.role != CR_POTRF && it.role != CR_TRSM) continue;
            if (it.n0 && expect[(size_t)(it.w0 - cbase)] != it.need0) bad = true;
            if (it.n1 && expect[(size_t)(it.w1 - cbase)] != it.need1) bad = true;
            if (it.role == CR_POTRF && it.w2 >= 0 && expect[(size_t)(it.w2 - cbase)] != it.need2) bad = true;
        }
    }
};

struct ScheduleBuilder {
    Symbolic &S;
    const ScheduleKnobs K;
    std::vector<i64> region_slots;          // split-K scratch slots needed per (stream group, side) region
    // structural-zero flags of a 128-row operand window [r0, r0 + TILE) of front s, one byte per K slab (step 13c), built on first use
    // (node-based map: the address of a flag vector stays valid while others are added -- a tile looks up two windows and keeps both pointers)
    std::vector<std::unordered_map<i32, std::vector<char>>> win_cache;
    std::vector<char> need_tmp;             // scratch of tile_skip_segments

    explicit ScheduleBuilder(Symbolic &S_) : S(S_), K(read_knobs()), win_cache(S_.fronts.size()) {}

    bool in_scope(i32 s, int g) const { return S.front_local[s] && !S.front_single[s] && (g < 0 || S.front_group[s] == g); }
    static void push_launch(std::vector<Launch> &L, Scope sc, i32 kind, i64 first, i64 count) {
        if (count > 0) L.push_back(Launch{kind, sc.group, first, count, sc.side, 0});
    }
    // ---------------- prologue ----------------
    void singles_and_upper_fronts() {
        // Isolated 1 x 1 fronts (an LP row that shares no column with any other row -- e.g. an inequality
        // row whose only entry is its slack: 13 % of the rows of the headline instance): one thread each in
        // k_single_factor / k_single_solve instead of a 256-thread workgroup in six different launches.
        S.front_single.assign(S.fronts.size(), 0);
        S.single_loff.clear(); S.single_dinvoff.clear(); S.single_col.clear();
        for (size_t s = 0; s < S.fronts.size(); ++s) {
            const FrontDesc &w = S.fronts[s];
            if (w.f == 1 && w.ns == 1 && w.nchild == 0 && w.parent < 0 && (i32)s != S.root_front) {
                S.front_single[s] = 1;
                if (S.front_local[s]) { S.single_loff.push_back(w.loff); S.single_dinvoff.push_back(w.dinvoff); S.single_col.push_back(w.col0); }
            }
        }
        // Step 13d (round 4): UPPER fronts.  On a block-angular LP 97 % of the factor's bytes are the panels of the diagonal blocks' top fronts (depth 1) and
        // the root, and nothing touches them before the extend-add of their level -- while the leaf levels below are a chain of short, latency-bound
        // launches that leave HBM idle.  Their zero-fill (0.9 ms of the 52 ms step on config C4, 2.4 of 137 ms on the north-star LP) and assembly therefore
        // run on a stream of their own beside the leaf levels; an LK_WAIT_UPPER marker makes a group's stream wait for them before its first launch
        // of an upper level.  Only with stream groups (the single-stream modes and graph replay keep the one-stream order).  TLPK_DEFER_UPPER=0: off.
        S.front_upper.assign(S.fronts.size(), 0);
        if (K.defer_upper && S.ngroups >= 2 && S.nlevels >= 3)
            for (size_t s = 0; s < S.fronts.size(); ++s) {
                const FrontDesc &w = S.fronts[s];
                if (S.front_local[s] && !S.front_fa[s] && !S.front_single[s] && S.depth[s] <= 1 && (i64)w.lda * w.ns > 4096) S.front_upper[s] = 1;
            }
    }
    // zero-fill of the panels before the assembly: per 64-column slice only the rows from the slice's first row down (the
    // blocks above the diagonal blocks are never read); the lower fronts first, then the upper ones
    void zero_fill_lists() {
        S.zero_tasks.clear(); S.zero_small.clear();
        for (int upper = 0; upper < 2; ++upper) {
            for (size_t s = 0; s < S.fronts.size(); ++s) {
                if (!S.front_local[s] || S.front_fa[s] || (int)S.front_upper[s] != upper) continue;       // (panels formed by k_front_assemble are written whole)
                const FrontDesc &w = S.fronts[s];
                if ((i64)w.lda * w.ns <= 4096) { S.zero_small.push_back((i32)s); continue; }      // whole panel by one wave
                for (i32 c0 = 0; c0 < w.ns; c0 += NB_IN) { S.zero_tasks.push_back((i32)s); S.zero_tasks.push_back(c0); }
            }
            if (!upper) S.n_zero_lower = (i64)S.zero_tasks.size() / 2;
        }
    }
    // ---------------- factorisation: assembly of a level ----------------
    // panels of the large fronts: tiles of FA_CW columns x <= 256 rows, every stored entry of the panel written exactly once
    // (rows from the first row of the column tile's 64-column slice down: what the packed panel stores)
    void front_assemble_tasks(const LevelPlan &P) {
        const i64 first = (i64)S.fa_tasks.size();
        for (i32 t = P.t0; t < P.t1; ++t) {
            const i32 s = S.level_fronts[t];
            if (!in_scope(s, P.g) || !S.front_fa[(size_t)s]) continue;
            const FrontDesc &w = S.fronts[s];
            const i32 npan = ea_npan(w, true), nbnd = ea_nbounds(w, true);
            for (i32 bc = 0; bc < npan; ++bc) {
                const i32 j0 = bc * FA_CW;
                for (i32 br0 = ((j0 >> 6) << 6) / FA_CW; br0 < nbnd - 1; br0 += FA_RB)
                    S.fa_tasks.push_back(FaTask{s, bc, br0, std::min(br0 + FA_RB, nbnd - 1)});
            }
        }
        push_launch(S.factor_launches, Scope{P.g, 0}, LK_FRONT_ASSEMBLE, first, (i64)S.fa_tasks.size() - first);
    }
    // extend-add.  Panel part (u_part = false): the children's update-matrix columns that land in the pivot
    // columns [0, ns) of their parent.  The U part [ns, f) is added AFTER the front's single
    // U update has written U (beta = 0), so U is never zero-filled nor read back by k_update.
    void extend_add_tasks(const LevelPlan &P, bool u_part) {
        const i64 first = (i64)S.ea_tasks.size();
        for (i32 t = P.t0; t < P.t1; ++t) {
            const i32 s = S.level_fronts[t];
            if (!in_scope(s, P.g)) continue;
            const FrontDesc &w = S.fronts[s];
            if (w.nchild == 0) continue;
            if (!u_part && S.front_fa[(size_t)s]) continue;      // panel part: k_front_assemble
            const i32 jbeg = u_part ? w.ns : 0, jend = u_part ? w.f : w.ns;
            const bool fa = S.front_fa[(size_t)s];
            const i32 cols = ea_cols(w, fa);
            i32 k = u_part ? ea_npan(w, fa) : 0;              // boundary index of j (section 13a)
            // TLPK_EA_BANDS (experiment): the rows of a big parent are cut into bands of whole boundary ranges, one workgroup per (column range, band)
            const i32 nbnd = ea_nbounds(w, fa);
            const i32 bands = (w.f >= 2048) ? K.ea_bands : 1;
            for (i32 j = jbeg; j < jend; j += cols, ++k) {
                if (bands == 1) { S.ea_tasks.push_back(EaTask{s, j, std::min(j + cols, jend), k, 0, 0, 0, 0}); continue; }
                // rows >= j only matter (lower triangle): bands over the boundaries [k, nbnd - 1)
                const i32 span = nbnd - 1 - k, per = (span + bands - 1) / bands;
                for (i32 b0 = k; b0 < nbnd - 1; b0 += std::max(per, 1)) S.ea_tasks.push_back(EaTask{s, j, std::min(j + cols, jend), k, b0, std::min(b0 + std::max(per, 1), nbnd - 1), 0, 0});
            }
        }
        push_launch(S.factor_launches, Scope{P.g, 0}, LK_EXTEND_ADD, first, (i64)S.ea_tasks.size() - first);
    }
    // ---------------- factorisation: update tiles ----------------
    // TLPK_SKIP_WIN (experiment): the window of rows a skip decision looks at, 128 (a tile's own rows) | 256 | 512: with a coarser window the tiles of a
    // super-tile skip the SAME slabs and keep walking K side by side (their operand loads meet in L2), at the price of fewer skipped slabs
    const char *window_flags(i32 s, i32 r0) {            // r0 = first row of a tile (NOT always a multiple of TILE: the tiles of U start at row ns)
        auto &lst = win_cache[(size_t)s];
        { const auto it = lst.find(r0); if (it != lst.end()) return it->second.data(); }
        const FrontDesc &w = S.fronts[s];
        const i64 nsl = (w.ns + 15) / 16, W = ((w.f + 15) / 16 + 63) / 64;
        const uint64_t *bits = S.skip_bits.data() + S.skip_off[(size_t)s];
        std::vector<char> fl((size_t)nsl, 0);
        // rows looked at: the tile's own [r0, r0 + TILE), widened to whole skip_win-row windows when skip_win > TILE
        const i32 lo = (K.skip_win > TILE) ? r0 / K.skip_win * K.skip_win : r0;
        const i32 hi = (K.skip_win > TILE) ? (r0 + TILE + K.skip_win - 1) / K.skip_win * K.skip_win : r0 + TILE;
        const i32 g0 = lo / 16, g1 = (std::min(hi, w.f) - 1) / 16;
        for (i64 k = 0; k < nsl; ++k) {
            const uint64_t *b = bits + k * W;
            char any = 0;
            for (i32 g = g0; g <= g1 && !any; ++g) any = (char)((b[g >> 6] >> (g & 63)) & 1);
            fl[(size_t)k] = any;
        }
        return lst.emplace(r0, std::move(fl)).first->second.data();
    }
    // K slabs in which both operand row ranges of the tile (rows i0.., rows j0..: the 128-row windows that hold them, never skipping a needed slab) have a
    // structural nonzero (step 13c), for a tile with at least two full slabs.  empty: the tile receives nothing.  Otherwise kexec = columns to execute,
    // and when slabs are skipped nsl = slabs to execute and, if `record`, seg = the tile's segment list in upd_seg.  min2: the 128 x 128 kernel's
    // pipeline wants >= 2 slabs (the last skipped ones are put back).
    struct Skip { i32 seg, nsl; double kexec; bool empty; };
    Skip tile_skip_segments(i32 s, i32 k0, i32 kw, i32 i0, i32 j0, i32 beta0, bool min2, bool record) {
        Skip sk{0, 0, (double)kw, false};
        const i32 nfull = kw / 16, sl0 = k0 / 16;
        const char *fi = window_flags(s, i0), *fj = window_flags(s, j0);
        i32 cnt = 0;
        for (i32 k = 0; k < nfull; ++k) cnt += (fi[sl0 + k] & fj[sl0 + k]);
        if (cnt == 0 && !beta0 && kw % 16 == 0) { sk.empty = true; return sk; }
        if (cnt == nfull) return sk;
        need_tmp.assign((size_t)nfull, 0);
        for (i32 k = 0; k < nfull; ++k) need_tmp[(size_t)k] = fi[sl0 + k] & fj[sl0 + k];
        if (min2) for (i32 k = nfull - 1; k >= 0 && cnt < 2; --k) if (!need_tmp[(size_t)k]) { need_tmp[(size_t)k] = 1; ++cnt; }
        sk.nsl = cnt; sk.kexec = 16.0 * cnt + kw % 16;
        if (!record) return sk;
        sk.seg = (i32)S.upd_seg.size() + 1;
        S.upd_seg.push_back(0);
        i32 nseg = 0;
        for (i32 k = 0; k < nfull;) {
            if (!need_tmp[(size_t)k]) { ++k; continue; }
            i32 e = k; while (e < nfull && need_tmp[(size_t)e]) ++e;
            S.upd_seg.push_back(k0 + 16 * k); S.upd_seg.push_back(e - k); ++nseg;
            k = e;
        }
        S.upd_seg[(size_t)sk.seg - 1] = nseg;
        return sk;
    }
    // one ts x ts tile (rows i0.., columns j0.. < c1) of front s with K = [k0, k0 + kw): counted, or pushed with its flops
    void push_tile(LevelPlan &P, const TileSink &sink, i32 s, const FrontDesc &w, i32 k0, i32 kw, i32 i0, i32 j0, i32 c1, i32 beta0, i32 ts) {
        const bool dry = sink.count != nullptr;
        Skip sk{0, 0, (double)kw, false};
        if (sink.skip && S.skip_off[(size_t)s] >= 0 && kw / 16 >= 2) sk = tile_skip_segments(s, k0, kw, i0, j0, beta0, ts == TILE, !dry);
        if (sk.empty) { if (!dry) S.flops_update_skipped += 2.0 * kw * tile_entries(w, i0, j0, c1, ts); return; }
        if (dry) { ++*sink.count; ++P.canon_count[(size_t)s]; return; }
        const double ent = tile_entries(w, i0, j0, c1, ts);
        S.flops_update += 2.0 * sk.kexec * ent; S.flops_update_skipped += 2.0 * (kw - sk.kexec) * ent;
        if (sink.chain) S.flops_update_chain += 2.0 * sk.kexec * ent;
        if (ts == TILE) S.update_tasks.push_back(UpdateTask{s, k0, kw, i0, j0, c1, beta0, 0, sk.seg, sk.nsl});
        else S.update_tasks.push_back(UpdateTask{s, k0, kw, i0, j0, c1, beta0, 0, sk.seg, sk.nsl, ts == 64 ? 1 : 2, 0});
        P.task_canon.push_back(P.canon_next[(size_t)s]++);
    }
    // The tiles of columns [c0, c1) of front s that receive K = [k0, k0 + kw).
    // part: 0 = only the tiles of the block column's diagonal block (rows < c0 + NB_OUT),
    //       1 = only the tiles below it, 2 = all
    // ts = 64 / 32 (chain launches only, part 0, K <= 256): the diagonal block's tiles as 64 x 64 tiles (UpdateTask.pad2 = 1, kernels.hip: update_tile64) or
    // 32 x 32 tiles (pad2 = 2, update_tile32: one 16 x 16 block per wave, operands straight from the panel) -- the short update that is left on the chain
    // behind a solved block column runs on ten / 36 CUs instead of three.  Same sums in the same order per entry.
    void push_update_region(LevelPlan &P, const TileSink &sink, i32 s, const FrontDesc &w, i32 k0, i32 kw, i32 c0, i32 c1, i32 beta0, int part, i32 ts = TILE) {
        if (kw <= 0 || c0 >= c1) return;
        if (ts < TILE) {
            for (i32 j0 = c0; j0 < c1; j0 += ts)
                for (i32 i0 = j0; i0 < std::min(c0 + NB_OUT, w.f); i0 += ts) push_tile(P, sink, s, w, k0, kw, i0, j0, c1, beta0, ts);
            return;
        }
        // tiles in super-tile order (UPD_SUPER x UPD_SUPER tiles): tasks that are neighbours in the list
        // read the same row / column slabs of the panel, and k_update deals runs of 64 consecutive
        // tasks to one XCD (one L2)
        const i32 SUP = K.upd_super * TILE;
        for (i32 J0 = c0; J0 < c1; J0 += SUP)
            for (i32 I0 = J0; I0 < w.f; I0 += SUP)
                for (i32 j0 = J0; j0 < std::min(J0 + SUP, c1); j0 += TILE)
                    for (i32 i0 = std::max(I0, j0); i0 < std::min(I0 + SUP, w.f); i0 += TILE) {
                        const bool diag_blk = i0 < c0 + NB_OUT;
                        if ((part == 0 && !diag_blk) || (part == 1 && diag_blk)) continue;
                        push_tile(P, sink, s, w, k0, kw, i0, j0, c1, beta0, TILE);
                    }
    }
    static bool pass_ok(const LevelPlan &P, int pass, i32 s) { return pass == PASS_ALL || ((bool)P.chain_front[(size_t)s] == (pass == PASS_CHAIN)); }
    // the fronts of the level a generator visits: this pass's fronts of the scope; dry runs see all of the rank's fronts of the level
    template <class F> void for_fronts(const LevelPlan &P, int pass, bool dry, F &&fn) {
        for (i32 t = P.t0; t < P.t1; ++t) {
            const i32 s = S.level_fronts[t];
            if (dry ? (bool)S.front_local[s] : (in_scope(s, P.g) && pass_ok(P, pass, s))) fn(s, S.fronts[s]);
        }
    }
    // a launch of the blocked factorisation: pushed, or (PASS_CHAIN) captured for build_chain
    void emit(LevelPlan &P, Scope sc, int pass, i32 kind, i64 first, i64 count) {
        if (count <= 0) return;
        if (pass == PASS_CHAIN) P.cap.push_back(Cap{kind, first, count}); else push_launch(S.factor_launches, sc, kind, first, count);
    }
    // ---------------- factorisation: one update launch ----------------
    // tiles the launch would have over ALL of the rank's fronts of the level (canon_count: per front)
    template <class Gen> i64 count_tiles(LevelPlan &P, Gen &&gen, bool skip) {
        i64 t_level = 0;
        for (i32 t = P.t0; t < P.t1; ++t) P.canon_count[(size_t)S.level_fronts[t]] = 0;
        gen(TileSink{&t_level, skip, false});
        return t_level;
    }
    void seed_canon(LevelPlan &P) {
        i64 acc = 0;
        for (i32 t = P.t0; t < P.t1; ++t) { const i32 s = S.level_fronts[t]; P.canon_next[(size_t)s] = acc; acc += P.canon_count[(size_t)s]; }
    }
    i32 splitk_parts(i64 t_level) const { return (t_level > 0) ? (i32)std::min<i64>(8, K.splitk_tiles / t_level) : 1; }
    // number of parts p in 1..8 that minimises the time of a wave of r equal tiles on tail_slots slots: ceil(r p / slots) / p
    i32 best_parts(i64 r) const {
        i32 best = 1; double tbest = (double)((r + K.tail_slots - 1) / K.tail_slots);
        for (i32 p = 2; p <= 8; ++p) {
            const double tp = (double)((r * p + K.tail_slots - 1) / K.tail_slots) / p;
            if (tp < tbest - 1e-9) { tbest = tp; best = p; }
        }
        return best;
    }
    // Longest first (TLPK_UPD_LPT, round 4): tiles that skip K slabs are shorter than their neighbours; dealt out last they fill the tail of
    // the launch instead of leaving long tiles to finish alone.  Stable: tiles of equal length keep the super-tile order (L2 locality).
    void lpt_order(LevelPlan &P, i64 f_upd, i64 cnt) {
        auto len = [](const UpdateTask &t) { return t.seg ? 16 * t.nsl + t.kw % 16 : t.kw; };
        std::vector<size_t> idx((size_t)cnt);
        std::iota(idx.begin(), idx.end(), 0);
        std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return len(S.update_tasks[(size_t)f_upd + a]) > len(S.update_tasks[(size_t)f_upd + b]); });
        std::vector<UpdateTask> tmp_t((size_t)cnt); std::vector<i64> tmp_c((size_t)cnt);
        for (size_t q = 0; q < (size_t)cnt; ++q) { tmp_t[q] = S.update_tasks[(size_t)f_upd + idx[q]]; tmp_c[q] = P.task_canon[idx[q]]; }
        std::copy(tmp_t.begin(), tmp_t.end(), S.update_tasks.begin() + f_upd);
        P.task_canon.swap(tmp_c);
    }
    // Round 6 (the review's tail shape): the chip holds 512 of a launch's 128 x 128 tiles at a time, and the r = tiles mod 512 tiles of the last round
    // take a whole round -- 18 % of the serialised update time of config C4 (tools/update_launch_eff.py: 5.96 of 32.96 ms).  When r is small the last
    // round's tiles are cut into their 64 x 64 quarters (UpdateTask.pad2 = 1, update_tile64: four waves per workgroup, four workgroups per CU): 4 r
    // quarter-length items on 1024 slots, launched right behind the full rounds.  Same K ranges / segment lists, every entry sums its K columns in the
    // same order: same bits (CPU emulator and device: tests/test_symbolic.py, tests/test_gpu_parity.py).  MEASURED (profiles/r06_tail64.txt) and OFF by default
    // (TLPK_TAIL64=288 turns it on): C4 52.5 vs 51.5 ms per step, north-star 138.0 vs 136.6, and the serialised `roofline.frac` FALLS (0.633 vs 0.638, north-star
    // 0.598 vs 0.620): a 128 x 128 tile that has its CU to itself in a half-empty last round runs at nearly twice the rate of two sharing the matrix pipes, the
    // four quarter tiles re-read the operands and pay a launch boundary.  Not for the side stream's diagonal tiles (few, and the single-stream modes merge them with the rows-below launch by task
    // range), not inside the dependency-driven launches (PASS_CHAIN: their items are already finer), not for launches of less than one round.
    void emit_whole_or_tail64(LevelPlan &P, Scope sc, int pass, i64 f_upd, i64 cnt) {
        i64 r = (K.tail64 > 0 && pass != PASS_CHAIN && sc.side == 0 && cnt >= K.tail64_slots) ? cnt % K.tail64_slots : 0;
        if (r > K.tail64) r = 0;
        if (r == 0) { emit(P, sc, pass, LK_UPDATE, f_upd, cnt); return; }
        std::vector<UpdateTask> tail(S.update_tasks.end() - r, S.update_tasks.end());
        S.update_tasks.resize(S.update_tasks.size() - (size_t)r);
        const i64 f_t64 = (i64)S.update_tasks.size();
        for (const UpdateTask &t : tail) {
            const FrontDesc &w = S.fronts[t.front];
            for (i32 dj = 0; dj < TILE; dj += 64)
                for (i32 di = 0; di < TILE; di += 64) {
                    const i32 si = t.i0 + di, sj = t.j0 + dj;
                    if (si >= w.f || sj >= t.jlim || si + 63 < sj) continue;      // outside the front / the column range / above the diagonal
                    S.update_tasks.push_back(UpdateTask{t.front, t.k0, t.kw, si, sj, t.jlim, t.beta0, 0, t.seg, t.nsl, 1, 0});
                }
        }
        emit(P, sc, pass, LK_UPDATE, f_upd, cnt - r);
        emit(P, sc, pass, LK_UPDATE_T64, f_t64, (i64)S.update_tasks.size() - f_t64);
    }
    // the tasks from f_upd on cut along K into parts that go to scratch slots, and the reductions that apply the parts in order: every tile into nsplit
    // parts (nsplit >= 2), or the tiles with canonical index >= tail_from into tail_parts, or (ksplit) every tile by K length
    void split_into_parts(LevelPlan &P, Scope sc, int pass, i64 f_upd, i32 nsplit, i64 tail_from, i32 tail_parts, bool ksplit) {
        std::vector<UpdateTask> orig(S.update_tasks.begin() + f_upd, S.update_tasks.end());
        S.update_tasks.resize(f_upd);
        const i64 f_red = (i64)S.reduce_tasks.size();
        i32 slot = (pass == PASS_CHAIN) ? (i32)P.chain_slot_base : 0;
        for (size_t q = 0; q < orig.size(); ++q) {
            const UpdateTask &t = orig[q];
            const i32 limit = (nsplit >= 2) ? nsplit : (P.task_canon[q] >= tail_from ? tail_parts : 1);
            const i32 parts = ksplit ? (t.pad2 ? 1 : std::min<i32>(8, (t.kw + K.ksplit_len - 1) / K.ksplit_len)) : std::min(limit, t.kw / 256);
            if (parts < 2) { S.update_tasks.push_back(t); continue; }
            const i32 base = (t.kw / parts) / 16 * 16;              // multiples of the kernel's K slab
            i32 k = 0;
            for (i32 sp = 0; sp < parts; ++sp) {
                const i32 kw_s = (sp == parts - 1) ? t.kw - k : base;
                S.update_tasks.push_back(UpdateTask{t.front, t.k0 + k, kw_s, t.i0, t.j0, t.jlim, t.beta0, slot + sp + 1});
                k += kw_s;
            }
            S.reduce_tasks.push_back(UpdateTask{t.front, slot, parts, t.i0, t.j0, t.jlim, t.beta0, 0});
            slot += parts;
        }
        // slots are relative to the scratch region of this launch's stream for now (see make_slots_absolute)
        const int region = (sc.group + 1) * 2 + sc.side;
        if ((int)region_slots.size() <= region) region_slots.resize(region + 1, 0);
        region_slots[region] = std::max<i64>(region_slots[region], slot);
        if (pass == PASS_CHAIN) P.chain_slot_base = slot;
        emit(P, sc, pass, LK_UPDATE, f_upd, (i64)S.update_tasks.size() - f_upd);
        emit(P, sc, pass, LK_UPDATE_REDUCE, f_red, (i64)S.reduce_tasks.size() - f_red);
    }
    // One update launch: `gen(sink)` pushes its tiles.  Split-K: when the launch would leave most of the
    // chip idle (fewer than ~128 tiles over ALL of the rank's fronts of the level -- the decision
    // must not depend on the stream groups), the K range of every tile is cut into up to 8 parts of
    // >= 256 columns, computed by different workgroups into scratch and applied in order by a
    // k_update_reduce launch.  A tile with K = 3300 runs for ~0.9 ms whatever runs beside it: with
    // 8 blocks per rank (8-GPU sharding), for the root front, and for the diagonal-block tiles on
    // the side stream this is the critical path.
    // Tail split (round 3, OFF by default: measured without gain).  The tiles of a launch have the same K, i.e. the same
    // duration T, and the chip holds 512 of them at a time (2 workgroups x 256 CUs): on paper a launch of 2.4 x 512 tiles takes
    // 3 T, the last T with 60 % of the slots empty, and cutting the r = (tiles mod slots) tiles of the last wave along K into
    // p parts (p minimising ceil(r p / slots) / p) lifts the simulated slot efficiency of the C4 schedule from 0.84 to 0.98.
    // On the device the update time did not move (32.1 -> 32.5 ms + 0.75 ms of reductions; profiles/r03_tail_split.txt): a
    // workgroup that has its CU to itself runs at nearly twice the rate of two sharing the matrix pipes, so a half-empty last
    // wave is not half idle.  TLPK_TAIL_SLOTS=512 turns the split on (tiles are chosen by their canonical index over ALL of
    // the rank's fronts of the level, so that results do not depend on the number of stream groups).
    template <class Gen> void emit_update_launch(LevelPlan &P, Scope sc, int pass, Gen &&gen) {
        const bool chain = pass == PASS_CHAIN;
        bool skip = true;
        i64 t_level = count_tiles(P, gen, skip);
        i32 nsplit = splitk_parts(t_level);
        if (nsplit >= 2 || K.tail_slots > 0) {           // split-K launches cut the K range by position: no skip lists there
            skip = false;
            t_level = count_tiles(P, gen, skip);
            nsplit = splitk_parts(t_level);
        }
        seed_canon(P);
        const i64 f_upd = (i64)S.update_tasks.size();
        P.task_canon.clear();
        gen(TileSink{nullptr, skip, chain});
        // Round 6, look-ahead levels (the levels the dependency-driven launch serves): NO item may run for longer than a link of the chain.  A tile with
        // K = 4096 holds its workgroup for 640 us -- four block columns of the chain -- and the block column that waits for it (its strips) stalls that long
        // whatever the number of tiles beside it.  Every tile of such a level is cut by K LENGTH, into parts of at most KSPLIT_LEN columns (<= 8 parts),
        // whatever the number of tiles in the launch; the reduction applies the parts in order.  (Split tiles take no skip lists: regenerate without them;
        // what the first generation added to the flop counts and to upd_seg stays.)
        bool ksplit = false;
        if (P.lookahead && K.ksplit_len > 0 && nsplit < 2 && K.tail_slots == 0) {
            for (i64 q = f_upd; q < (i64)S.update_tasks.size(); ++q) if (S.update_tasks[(size_t)q].kw > K.ksplit_len && !S.update_tasks[(size_t)q].pad2) { ksplit = true; break; }
            if (ksplit) {
                S.update_tasks.resize((size_t)f_upd);
                P.task_canon.clear();
                seed_canon(P);
                gen(TileSink{nullptr, false, chain});
            }
        }
        const i64 cnt = (i64)S.update_tasks.size() - f_upd;
        if (cnt == 0) return;
        if (K.upd_lpt && nsplit < 2 && K.tail_slots == 0) lpt_order(P, f_upd, cnt);
        i64 tail_from = t_level; i32 tail_parts = 1;      // tiles with canonical index >= tail_from are cut into tail_parts
        if (nsplit < 2 && K.tail_slots > 0 && t_level > 0) {
            const i64 r = t_level % K.tail_slots;
            if (t_level < K.tail_slots) nsplit = best_parts(t_level);                    // a single, partly filled wave: cut every tile
            else if (r > 0) { tail_parts = best_parts(r); tail_from = t_level - r; }  // the last wave
        }
        if (nsplit < 2 && tail_parts < 2 && !ksplit) emit_whole_or_tail64(P, sc, pass, f_upd, cnt);
        else split_into_parts(P, sc, pass, f_upd, nsplit, tail_from, tail_parts, ksplit);
    }
    // ---------------- factorisation: the plan of a level ----------------
    // the rank's fronts of the level with more than one block column: how many, and the widest (the look-ahead rule and the chain rule; never the stream groups)
    std::pair<i32, i32> big_fronts(const LevelPlan &P) const {
        i32 nbig = 0, ns_max = 0;
        for (i32 t = P.t0; t < P.t1; ++t) {
            const i32 sf = S.level_fronts[t];
            if (!S.front_local[sf] || S.front_single[sf]) continue;
            if (S.fronts[sf].ns > NB_OUT) { ++nbig; ns_max = std::max(ns_max, S.fronts[sf].ns); }
        }
        return {nbig, ns_max};
    }
    // Look-ahead for the diagonal blocks (round 4).  The chain potrf(io) -> trsm(io) -> [update of the diagonal block of io + 1] -> potrf(io + 1) is
    // the critical path of a level with one big front (pds-class LPs: 31 block columns), of the root front, and of every rank of a sharded job.
    // The left-looking update of that diagonal block had K = [0, ko + 256): a few tiles with K up to the whole front, cut by split-K and followed by a
    // reduction -- 0.15 .. 0.3 ms on the chain per block column.  Now the part K = [k_first, ko) (everything but the block column just finished) rides in
    // the rows-below launch of block column io (same operands, same readiness: block columns < io), off the chain; behind trsm(io) only
    // K = [ko, ko + 256) is left: 3 tiles x 16 slabs.
    // MEASURED (profiles/r04_lookahead.txt) and OFF by default (TLPK_LOOKAHEAD=1 turns it on): pds-class LP 18.86 -> 18.5 ms per step -- split-K had already
    // cut the long-K diagonal update to ~0.1 ms and the chain is the potrf kernel itself (7.8 of 13.8 ms) --, C4 / north-star LP unchanged, and the C3
    // shape LOSES 11 % (675 -> 750 ms: inside its 16-wide macro columns the look-ahead tiles are a second long-K tail in every rows-below launch).
    // Round 5: AUTO (TLPK_LOOKAHEAD unset) turns it on for the levels it was measured to help -- at most 16 of this rank's fronts have more than
    // one block column and none has more than 12 288 pivot columns (a pds-class top front, the root front, the few blocks of a rank of an
    // 8-GPU job; not the C3 shape's 48 000-column front, not the 32 blocks per stream group of config C4 at N = 1, whose diagonal-block chains
    // are hidden behind the bulk updates anyway).  The rule looks at the rank's fronts of the level only, never at the stream groups.
    bool lookahead_rule(const LevelPlan &P) const {
        if (K.lookahead >= 0) return K.lookahead == 1;
        const auto [nbig, ns_max] = big_fronts(P);
        return nbig >= 1 && nbig <= 16 && ns_max <= 12288;
    }
    // Macro columns: G consecutive block columns share ONE left-looking update with
    // K = [0, kM) (kM = first column of the macro column); inside the macro column a block
    // column only adds the short update K = [kM, ko).  G is chosen at the start of every macro
    // column so that the long-K launch has >= ~2000 tiles (4 waves of the chip): G = 1 (every
    // block column pulls all previous columns itself) while a block-column launch is that big
    // anyway; a level with a single huge front (general sparse LPs), and the last block columns
    // of any level, get wider macro columns -- a tile with K = 40 000 runs for 10 ms whatever
    // the number of tiles beside it.  G depends on all of this rank's fronts of the level, not only
    // on the current stream group's: the rounding must not depend on the number of streams
    // (across rank counts the all-reduce order differs anyway; a rank with few blocks needs the
    // wider macro columns to fill its GPU).
    i32 macro_width(const LevelPlan &P, i32 ko) const {
        constexpr i32 G_MAX = 16;
        i64 tiles_bc = 0;
        for (i32 t = P.t0; t < P.t1; ++t) {
            if (!S.front_local[S.level_fronts[t]]) continue;
            const FrontDesc &w = S.fronts[S.level_fronts[t]];
            if (w.ns > ko + NB_OUT) tiles_bc += 2 * (i64)((w.f - ko + TILE - 1) / TILE);
        }
        // launches of >= ~1000 tiles are left alone (measured on C4: macro columns there cost 0.3 ms,
        // two stream groups already fill each other's tails)
        if (tiles_bc <= 0 || 2 * tiles_bc >= K.macro_tiles) return (i32)1;
        // (TLPK_LA_MACRO=0, diagnostics: no macro columns on the look-ahead levels -- every block column pulls K = [0, ko - 256) one block column early.
        // Measured WORSE, pds-class 13.8 -> 14.6 ms: in the middle of a 7 900-column front a block column's update is 130 us of the whole chip, as long as a
        // link of the chain; the macro columns do that work early, while the chain is latency-bound, the pure left-looking form does it when it is due.)
        if (P.lookahead && !K.la_macro) return (i32)1;
        return (i32)std::min<i64>(G_MAX, (K.macro_tiles + tiles_bc - 1) / tiles_bc);
    }
    void macro_columns(LevelPlan &P) const {
        P.mac_first.assign((size_t)P.nouter + 2, 0); P.mac_G.assign((size_t)P.nouter + 2, 1);
        i32 G = 1, io_macro = 0;
        for (i32 io = 0; io <= P.nouter + 1; ++io) {
            if (io >= io_macro + G) { io_macro = io; G = macro_width(P, io * NB_OUT); }
            else if (io == 0) G = macro_width(P, 0);
            P.mac_first[(size_t)io] = io_macro; P.mac_G[(size_t)io] = G;
        }
    }
    // TLPK_CHAIN: 0 = off, 1 = every level that has a front with more than one block column, unset = auto: the levels the look-ahead rule names
    // (at most TLPK_CHAIN_MAX_FRONTS = 8 of this rank's fronts have more than one block column, none more than 12 288 pivot columns).  The chain's
    // diagonal-block role is the round-5 DPP kernel: the older block kernels (TLPK_POTRF_MODE != 3, diagnostics) keep the launches.
    // ... and the widest of them has at least TLPK_CHAIN_MIN_NS pivot columns: a front of two or three block columns has too few items for the hand-overs
    // (a few microseconds each) to beat the launches it replaces (25fv47-class LPs; the lower levels of a pds-class LP)
    // Marks the level's chain fronts; true when one of them is in the scope.
    bool chain_rule(LevelPlan &P) {
        const auto [nbig, ns_big] = big_fronts(P);
        const bool use_chain = K.chain != 0 && K.potrf_default && K.tail_slots == 0 && nbig >= 1 &&
                               (K.chain > 0 || (nbig <= K.chain_max_fronts && ns_big <= 12288 && ns_big >= K.chain_min_ns));
        bool any = false;
        if (!use_chain) return any;
        for (i32 t = P.t0; t < P.t1; ++t) {
            const i32 sf = S.level_fronts[t];
            if (S.front_local[sf] && !S.front_single[sf] && S.fronts[sf].ns > NB_OUT) { P.chain_front[(size_t)sf] = 1; any = any || in_scope(sf, P.g); }
            if (P.chain_front[(size_t)sf] && in_scope(sf, P.g)) {       // the algorithmic update flops of its columns (the formula of step 12) now run inside k_chain
                const FrontDesc &w = S.fronts[sf];
                for (i32 c = 0; c < w.ns; ++c) {
                    const double l = (double)S.colcount[w.col0 + c] - (double)(std::min((c / NB_OUT + 1) * NB_OUT, w.ns) - c);
                    if (l > 0) S.flops_update_alg_chain += l * l;
                }
            }
        }
        return any;
    }
    // ---------------- factorisation: the block columns of a level ----------------
    // the diagonal blocks of block column ko: narrow blocks (one 64-wide step) and wide ones go to different kernels
    // (and the fronts with <= SMALL_NS pivot columns -- most fronts of the leaf levels -- take one
    // wave per front, four fronts per workgroup, list padded with front = -1)
    void potrf_launches(LevelPlan &P, Scope sc, int pass, i32 ko) {
        for (int cls = 0; cls < 3; ++cls) {              // 0 small, 1 narrow, 2 wide
            const i64 f_potrf = (i64)S.potrf_tasks.size();
            for_fronts(P, pass, false, [&](i32 s, const FrontDesc &w) {
                if (ko >= w.ns) return;
                const i32 no = std::min(NB_OUT, w.ns - ko);
                const int c = (w.ns <= SMALL_NS) ? 0 : (no > NB_IN ? 2 : 1);
                if (c == cls) S.potrf_tasks.push_back(PotrfTask{s, ko, no, ko});
            });
            if (cls == 0) {
                while (((i64)S.potrf_tasks.size() - f_potrf) % 4) S.potrf_tasks.push_back(PotrfTask{-1, 0, 0, 0});
                emit(P, sc, pass, LK_POTRF_SMALL, f_potrf, ((i64)S.potrf_tasks.size() - f_potrf) / 4);
            } else
                emit(P, sc, pass, cls == 2 ? LK_POTRF_WIDE : LK_POTRF, f_potrf, (i64)S.potrf_tasks.size() - f_potrf);
        }
    }
    // k_trsm solves the rows below the diagonal block in one pass
    // (thin block columns -- the small fronts of the leaf levels -- take one thread per row instead
    // of 16-row MFMA strips that would be 90 % padding)
    void trsm_launches(LevelPlan &P, Scope sc, int pass, i32 ko) {
        for (int thin = 0; thin < 2; ++thin) {
            const i64 f_trsm = (i64)S.trsm_tasks.size();
            for_fronts(P, pass, false, [&](i32 s, const FrontDesc &w) {
                if (ko >= w.ns) return;
                const i32 no = std::min(NB_OUT, w.ns - ko);
                if ((no <= TRSM_THIN_W && pass != PASS_CHAIN) != (thin == 1)) return;      // (chain items: 64-row strips for every width)
                const i32 step = thin ? 256 : TRSM_WG_ROWS;
                // row ranges END on multiples of `step` rows (16-row strips then sit on 128-byte lines of the
                // line-aligned panel); pad1 = row limit of the task
                for (i32 r0 = ko + no; r0 < w.f;) {
                    const i32 r1 = std::min(w.f, (r0 / step + 1) * step);
                    S.trsm_tasks.push_back(TrsmTask{s, ko, no, r0, ko, 0, r1, 0});
                    r0 = r1;
                }
            });
            emit(P, sc, pass, thin ? LK_TRSM_THIN : LK_TRSM, f_trsm, (i64)S.trsm_tasks.size() - f_trsm);
        }
    }
    // Blocked partial factorisation.  Outer level LEFT-looking: before the 256-wide block
    // column `io` of a front is factorised, one MFMA update accumulates the contribution of
    // ALL previous columns [0, ko) in registers and writes each target entry once (the
    // right-looking variant re-wrote the whole trailing matrix every 256 columns and was
    // HBM-bound on that read-modify-write).  The update matrix U gets a single update with
    // K = [0, ns) after the last block column.
    void block_columns(LevelPlan &P, int pass) {
        i32 pmax = 0;
        for (i32 t = P.t0; t < P.t1; ++t) if (in_scope(S.level_fronts[t], P.g) && pass_ok(P, pass, S.level_fronts[t])) pmax = std::max(pmax, S.fronts[S.level_fronts[t]].ns);
        if (pmax == 0 && pass != PASS_ALL) return;
        const i32 nouter = (pass == PASS_ALL) ? P.nouter : (pmax + NB_OUT - 1) / NB_OUT;      // block columns of THIS pass's fronts (the macro tables cover the level's)
        const bool chain = pass == PASS_CHAIN, la_full = K.la_full, lookahead = P.lookahead;
        for (i32 io = 0; io <= nouter; ++io) {
            const i32 ko = io * NB_OUT;
            const i32 io_macro = P.mac_first[(size_t)io], G = P.mac_G[(size_t)io];
            const i32 gi = io - io_macro, kM = io_macro * NB_OUT;
            // Round 6, with the look-ahead: the FIRST block column of a macro column (gi == 0) used to pull all of K = [0, ko) itself -- tiles of up to 4096 columns
            // (450 - 600 us each) between strips(io - 1) and strips(io), ON the chain (profiles/r06_chain_trace_pds.txt: one 450 us stall per macro column start).
            // Now K = [0, ko - 256) comes with block column io - 1 (same operands, ready one block column earlier, off the chain) for the whole block column, not
            // only for its diagonal block; behind strips(io - 1) only the short K = [ko - 256, ko) is left, as for every other block column.
            // TLPK_LA_FULL=1 (diagnostics): the same for EVERY block column of a look-ahead level (inside the first macro column K = [0, ko) grows with ko).
            const bool mac_la = lookahead && io >= 2 && (gi == 0 || la_full);
            const i32 ka_base = (gi == 0) ? 0 : kM;
            const i32 ka = mac_la ? std::max(ka_base, ko - NB_OUT) : ka_base;       // this block column still needs K = [ka, ko)
            const i32 kd = lookahead ? std::max(ka, ko - NB_OUT) : ka;      // ... its diagonal block only K = [kd, ko): the rest came with block column io - 1
            // Block column io.  The left-looking update of its DIAGONAL block and the factorisation
            // of that block (k_potrf*: a serial chain inside one workgroup per front) go to the
            // group's side stream; the update of the rows below runs concurrently on the group's
            // stream and hides them.  Only stream order and events: correct under any scheduling
            // (a profiler that serialises dispatches included).
            const bool overlap = io > 0 && io < nouter;
            const bool fork = overlap && !chain;
            const Scope main{P.g, 0}, side{P.g, fork ? 1 : 0};
            if (fork) S.factor_launches.push_back(Launch{LK_SIDE_FORK, P.g, 0, 0, 0, 0});
            if (overlap)
                emit_update_launch(P, side, pass, [&](const TileSink &sink) {
                    const bool dry = sink.count != nullptr;
                    for_fronts(P, pass, dry, [&](i32 s, const FrontDesc &w) {
                        if (ko < w.ns) push_update_region(P, sink, s, w, kd, ko - kd, ko, std::min(ko + NB_OUT, w.ns), 0, 0, (chain && !dry && ko - kd <= NB_OUT) ? K.chain_tile : TILE);
                    });
                });
            if (io < nouter) potrf_launches(P, side, pass, ko);
            // rows below the diagonal block; at the start of a macro column also the other block
            // columns of the macro column (K = [0, kM)); past the last block column of a front,
            // U = -L21 L21' (written)
            emit_update_launch(P, main, pass, [&](const TileSink &sink) {
                for_fronts(P, pass, sink.count != nullptr, [&](i32 s, const FrontDesc &w) {
                    const i32 my_nouter = (w.ns + NB_OUT - 1) / NB_OUT;
                    if (io < my_nouter) {
                        push_update_region(P, sink, s, w, ka, ko - ka, ko, std::min(ko + NB_OUT, w.ns), 0, overlap ? 1 : 2);
                        if (gi == 0 && G > 1)
                            push_update_region(P, sink, s, w, 0, kM, ko + NB_OUT, std::min(kM + G * NB_OUT, w.ns), 0, 2);
                        // look-ahead: the diagonal block of block column io + 1, K = [k_first(io + 1), ko)
                        if (lookahead && io >= 1 && io + 1 < my_nouter) {
                            const i32 k1 = P.k_first(io + 1);
                            // (the next block column starts a macro column: the whole block column, see mac_la above)
                            if (ko > k1) push_update_region(P, sink, s, w, k1, ko - k1, ko + NB_OUT, std::min(ko + 2 * NB_OUT, w.ns), 0, (la_full || P.mac_first[(size_t)io + 1] == io + 1) ? 2 : 0);
                        }
                    } else if (io == my_nouter) push_update_region(P, sink, s, w, 0, w.ns, w.ns, w.f, 1, 2);
                });
            });
            if (fork) S.factor_launches.push_back(Launch{LK_SIDE_JOIN, P.g, 0, 0, 0, 0});
            if (io == nouter) break;
            trsm_launches(P, main, pass, ko);
        }
    }
    // the captured launches of PASS_CHAIN as the items of one LK_CHAIN launch (ChainBuilder, above)
    void build_chain(LevelPlan &P) {
        if (P.cap.empty()) return;
        ChainBuilder C(S, K.chain_jit, !S.shared_device && K.chain_early);
        i64 ncnt = 0;
        for (i32 t = P.t0; t < P.t1; ++t) {
            const i32 s = S.level_fronts[t];
            if (!in_scope(s, P.g) || !P.chain_front[(size_t)s]) continue;
            const FrontDesc &w = S.fronts[s];
            ChainBuilder::FC c; c.base = ncnt; c.nbc = (w.ns + NB_OUT - 1) / NB_OUT; c.ntr = (w.f + TILE - 1) / TILE; c.nsl = (w.f + 63) / 64;
            c.stride = 5 + 2 * c.ntr + c.nsl;
            ncnt += (i64)c.nbc * c.stride;
            C.fc[s] = c;
        }
        const i64 ticket_idx = S.chain_counters, first_item = (i64)S.chain_items.size();
        C.cbase = S.chain_counters + 1;
        C.expect.assign((size_t)ncnt, 0);
        C.run(P.cap, first_item);
        if (C.bad) { S.error = "internal: inconsistent chain schedule"; return; }
        S.factor_launches.push_back(Launch{LK_CHAIN, P.g, first_item, (i64)S.chain_items.size() - first_item, 0, (i32)ticket_idx});
        S.chain_counters += 1 + (i64)C.expect.size();
    }
    // one level of stream group g (-1: the depth-0 fronts)
    void factor_level(int g, i32 d) {
        LevelPlan P{g, S.level_ptr[d], S.level_ptr[d + 1]};
        bool any_upper = false;
        for (i32 t = P.t0; t < P.t1 && !any_upper; ++t) any_upper = in_scope(S.level_fronts[t], g) && S.front_upper[(size_t)S.level_fronts[t]];
        if (any_upper) S.factor_launches.push_back(Launch{LK_WAIT_UPPER, g, (i64)g, 0, 0, 0});      // step 13d (`first` repeats the group: the exported triples carry no group)
        front_assemble_tasks(P);
        extend_add_tasks(P, false);                      // (a) panel part
        if (d == 0 && S.root_front >= 0) S.factor_launches.push_back(Launch{LK_ALLREDUCE_ROOT, -1, 0, 0});
        // (b) the block columns
        for (i32 t = P.t0; t < P.t1; ++t) if (in_scope(S.level_fronts[t], g)) P.max_ns = std::max(P.max_ns, S.fronts[S.level_fronts[t]].ns);
        P.nouter = (P.max_ns + NB_OUT - 1) / NB_OUT;
        P.canon_count.assign(S.fronts.size(), 0); P.canon_next.assign(S.fronts.size(), 0);
        P.chain_front.assign(S.fronts.size(), 0);
        P.lookahead = lookahead_rule(P);
        macro_columns(P);
        if (!chain_rule(P)) block_columns(P, PASS_ALL);
        else {
            block_columns(P, PASS_LAUNCH);
            P.cap.clear(); P.chain_slot_base = 0;
            block_columns(P, PASS_CHAIN);
            build_chain(P);
        }
        extend_add_tasks(P, true);                       // (c) U part (every U of this level has been written by now)
    }
    // split-K scratch: every stream (group x side) gets its own region, launches of one stream reuse it;
    // make the slot numbers absolute
    void make_slots_absolute() {
        std::vector<i64> base(region_slots.size() + 1, 0);
        for (size_t r = 0; r < region_slots.size(); ++r) base[r + 1] = base[r] + region_slots[r];
        S.spart_len = base.back() * (i64)TILE * TILE;
        for (const Launch &L : S.factor_launches) {
            if (L.kind != LK_UPDATE && L.kind != LK_UPDATE_REDUCE) continue;
            const size_t region = (size_t)((L.group + 1) * 2 + L.side);
            if (region >= region_slots.size() || base[region] == 0) continue;
            for (i64 q = L.first; q < L.first + L.count; ++q) {
                if (L.kind == LK_UPDATE) { if (S.update_tasks[q].pad1) S.update_tasks[q].pad1 += (i32)base[region]; }
                else S.reduce_tasks[q].k0 += (i32)base[region];
            }
        }
        for (const Launch &L : S.factor_launches) {              // the split-K tasks inside the chain launches (region of the group's main stream)
            if (L.kind != LK_CHAIN) continue;
            const size_t region = (size_t)((L.group + 1) * 2);
            if (region >= region_slots.size() || base[region] == 0) continue;
            for (i64 q = L.first; q < L.first + L.count; ++q) {
                const ChainItem &it = S.chain_items[(size_t)q];
                if (it.role == CR_UPDATE) { if (S.update_tasks[(size_t)it.task].pad1) S.update_tasks[(size_t)it.task].pad1 += (i32)base[region]; }
                else if (it.role == CR_REDUCE && it.sub == 0) S.reduce_tasks[(size_t)it.task].k0 += (i32)base[region];
            }
        }
    }
    // ---------------- solves ----------------
    // (thin but TALL fronts keep the workgroup-per-row-chunk kernels: one wave walking 1000 rows is slower)
    bool is_small(i32 s) const { return S.fronts[s].ns <= SMALL_NS && S.fronts[s].f - S.fronts[s].ns <= SMALL_ROWS && s != S.root_front; }
    // Persistent sweeps (default): the block steps of a level's triangular solves run inside ONE launch per
    // direction; a solved SOLVE_NB-wide block is handed to the workgroups that need it through a flag word
    // per (front, block).  TLPK_SWEEP=0 keeps one launch per block step (the round-1 schedule).
    void solve_flags() {
        S.sweep = K.sweep;
        S.n_sweep_flags = 0;
        for (size_t s = 0; s < S.fronts.size(); ++s) {
            FrontDesc &w = S.fronts[s];
            w.flagoff = -1;
            if (!S.front_local[s] || S.front_single[s] || is_small((i32)s)) continue;
            w.flagoff = 0;                       // handled by the sweep kernels (hand-over words are indexed by column)
            S.n_sweep_flags += 1;
        }
    }
    // small fronts (<= SMALL_NS pivot columns: most fronts of the leaf levels): diagonal solve and
    // update of the rows below by ONE wave per front, four fronts per workgroup (a 256-thread
    // workgroup per front and kernel is mostly fixed latency); padded to a multiple of 4.  Returns (first task, groups of four).
    std::pair<i64, i64> small_front_list(int g, i32 t0, i32 t1, std::vector<SolveTask> &small) {
        const i64 first = (i64)small.size();
        for (i32 t = t0; t < t1; ++t) {
            const i32 s = S.level_fronts[t];
            if (in_scope(s, g) && is_small(s)) small.push_back(SolveTask{s, 0, S.fronts[s].ns, 0, 0, 0, 0, 0});
        }
        while (((i64)small.size() - first) % 4) small.push_back(SolveTask{-1, 0, 0, 0, 0, 0, 0, 0});
        return {first, ((i64)small.size() - first) / 4};
    }
    i32 max_ns_not_small(int g, i32 t0, i32 t1) const {
        i32 max_ns = 0;
        for (i32 t = t0; t < t1; ++t) if (in_scope(S.level_fronts[t], g) && !is_small(S.level_fronts[t])) max_ns = std::max(max_ns, S.fronts[S.level_fronts[t]].ns);
        return max_ns;
    }
    // The two launches of a level and direction under TLPK_SWEEP: its small fronts and its sweep (items from sweep_first on).
    // Round 6: on a level whose sweep is small (at most TLPK_SOLVE_MERGE = 256 items) the small fronts ride in the sweep's launch, as items of their own behind
    // the sweep's (forward: slot = 2, backward: nslot = -2; k0 = a group of four small-front tasks; no dependencies: any ticket will do) -- one launch per level
    // and direction less where a launch costs more than the fronts in it.  Same bodies, same arithmetic.
    // Round 6: the small fronts of a level beside its sweep (the group's side stream, forked behind the gather and joined in front of the next level's gather)
    // when the level has both: different fronts of one level, nothing in common but the gathered right-hand side.  One launch off the level's chain -- what a
    // latency-bound LP pays per launch, and on the north-star LP the small-front kernels were 0.8 of the 6.5 ms of a solve.
    // (TLPK_SOLVE_SIDE=1, experiment, OFF: measured neutral on C4 / north-star -- 51.6 vs 51.5, 136.3 vs 136.5 ms -- and SLOWER on the latency-bound LPs, 25fv47 class 1.17
    // vs 0.99 ms, pds class 14.05 vs 13.83: a fork / join costs more than the launch it takes off the chain; profiles/r06_solve_side.txt)
    void small_and_sweep_launches(int g, bool fwd, i64 small_first, i64 small_count, i64 sweep_first) {
        std::vector<SolveTask> &small = fwd ? S.fwd_small_tasks : S.bwd_small_tasks, &sweep = fwd ? S.fwd_sweep_tasks : S.bwd_sweep_tasks;
        std::vector<Launch> &L = fwd ? S.fwd_launches : S.bwd_launches;
        i64 sweep_count = (i64)sweep.size() - sweep_first;
        bool merged = false;
        if (K.solve_merge > 0 && small_count > 0 && sweep_count > 0 && sweep_count <= K.solve_merge) {
            for (i64 q = 0; q < small_count; ++q) {
                i32 fr = -1;
                for (int u = 0; u < 4; ++u) if (small[(size_t)(small_first + 4 * q + u)].front >= 0) { fr = small[(size_t)(small_first + 4 * q + u)].front; break; }
                sweep.push_back(SolveTask{fr, (i32)(small_first / 4 + q), 0, 0, fwd ? 2 : 0, fwd ? 0 : -2, 0, 0});
            }
            sweep_count += small_count; small_count = 0; merged = true;
        }
        const bool beside = K.solve_side && small_count > 0 && sweep_count > 0;
        if (beside) L.push_back(Launch{LK_SIDE_FORK, g, 0, 0, 0, 0});
        push_launch(L, Scope{g, beside ? 1 : 0}, fwd ? LK_FWD_SMALL : LK_BWD_SMALL, small_first, small_count);
        push_launch(L, Scope{g, 0}, fwd ? LK_FWD_SWEEP : LK_BWD_SWEEP, sweep_first, sweep_count);
        if (merged) L.back().pad = 1;
        if (beside) L.push_back(Launch{LK_SIDE_JOIN, g, 0, 0, 0, 0});
    }
    void fwd_gather_launch(int g, i32 t0, i32 t1) {
        const i64 first = (i64)S.fwd_gather_tasks.size();
        for (i32 t = t0; t < t1; ++t) {
            const i32 s = S.level_fronts[t];
            if (!in_scope(s, g)) continue;
            const FrontDesc &w = S.fronts[s];
            if (w.nchild == 0 && w.f == w.ns) continue;
            // leaves only clear their contribution vector (rows >= ns)
            // nb = rows of the task: 256 (one thread per row), or 32 = 8 lanes per row for a front whose rows collect many
            // entries each (the root front of a block-angular LP: one per diagonal block)
            const double per_row = (double)(S.gth_ptr[(size_t)w.rowoff + w.f] - S.gth_ptr[(size_t)w.rowoff]) / std::max(1, w.f);
            const i32 step = (per_row >= GATHER_WIDE_PER_ROW) ? SOLVE_ROWS / 8 : SOLVE_ROWS;
            for (i32 r0 = (w.nchild == 0) ? (w.ns / SOLVE_ROWS) * SOLVE_ROWS : 0; r0 < w.f; r0 += step)
                S.fwd_gather_tasks.push_back(SolveTask{s, 0, step, r0, 0, 0, 0, 0});
        }
        push_launch(S.fwd_launches, Scope{g, 0}, LK_FWD_GATHER, first, (i64)S.fwd_gather_tasks.size() - first);
    }
    // Items in hand-out order (workgroups draw them from a ticket counter): chunk index first, front
    // second, so that an item only ever waits for items with a smaller ticket -- those are held by
    // workgroups that are already running, whatever the dispatch order (no deadlock), and the fronts of
    // the level advance side by side.
    void fwd_sweep_items(int g, i32 t0, i32 t1) {
        i32 max_chunks = 0;
        for (i32 t = t0; t < t1; ++t) {
            const i32 s = S.level_fronts[t];
            if (!in_scope(s, g) || is_small(s)) continue;
            const FrontDesc &w = S.fronts[s];
            max_chunks = std::max(max_chunks, (w.ns + SWEEP_NB - 1) / SWEEP_NB + (w.f > w.ns ? (w.f + SOLVE_NB - 1) / SOLVE_NB - w.ns / SOLVE_NB : 0));
        }
        for (i32 ci = 0; ci < max_chunks; ++ci)
            for (i32 t = t0; t < t1; ++t) {
                const i32 s = S.level_fronts[t];
                if (!in_scope(s, g) || is_small(s)) continue;
                const FrontDesc &w = S.fronts[s];
                const i32 nblk = (w.ns + SWEEP_NB - 1) / SWEEP_NB;
                if (ci < nblk) S.fwd_sweep_tasks.push_back(SolveTask{s, ci * SWEEP_NB, std::min(SWEEP_NB, w.ns - ci * SWEEP_NB), 0, 1, ci, 0, 0});
                else {
                    // rows below the pivot block in chunks that END on multiples of SOLVE_NB rows (line-aligned loads;
                    // only the first chunk of a front is ragged)
                    const i32 q = ci - nblk;
                    const i32 r0 = (q == 0) ? w.ns : (w.ns / SOLVE_NB + q) * SOLVE_NB;
                    const i32 r1 = std::min(w.f, (w.ns / SOLVE_NB + q + 1) * SOLVE_NB);
                    if (r0 < w.f) S.fwd_sweep_tasks.push_back(SolveTask{s, r0, r1 - r0, 0, 0, nblk, 0, 0});
                }
            }
    }
    // forward solve of one level: gather, small fronts, then the sweep -- or (TLPK_SWEEP=0) one diagonal + update launch pair per 128-column block step
    void fwd_level(int g, i32 d) {
        const i32 t0 = S.level_ptr[d], t1 = S.level_ptr[d + 1];
        fwd_gather_launch(g, t0, t1);
        if (d == 0 && S.root_front >= 0) S.fwd_launches.push_back(Launch{LK_ALLREDUCE_ROOT, -1, 0, 0});
        const auto [small_first, small_count] = small_front_list(g, t0, t1, S.fwd_small_tasks);
        if (S.sweep) {
            const i64 first = (i64)S.fwd_sweep_tasks.size();
            fwd_sweep_items(g, t0, t1);
            small_and_sweep_launches(g, true, small_first, small_count, first);
            return;
        }
        push_launch(S.fwd_launches, Scope{g, 0}, LK_FWD_SMALL, small_first, small_count);      // (in stream order)
        const i32 max_ns = max_ns_not_small(g, t0, t1);
        for (i32 kb = 0; kb < max_ns; kb += SOLVE_NB) {
            const i64 f_diag = (i64)S.fwd_diag_tasks.size(), f_upd = (i64)S.fwd_update_tasks.size();
            // round 0: the look-ahead workgroups (first row chunk: they also solve the next diagonal
            // block) of every front, so that they start with the launch; round 1: the other chunks
            for (int round = 0; round < 2; ++round)
            for (i32 t = t0; t < t1; ++t) {
                const i32 s = S.level_fronts[t];
                if (!in_scope(s, g) || is_small(s)) continue;
                const FrontDesc &w = S.fronts[s];
                if (kb >= w.ns) continue;
                const i32 nb = std::min(SOLVE_NB, w.ns - kb);
                const i32 next_nb = std::min(SOLVE_NB, w.ns - (kb + nb));      // <= 0: last block
                if (round == 0 && kb == 0) S.fwd_diag_tasks.push_back(SolveTask{s, kb, nb, 0, 0, 0, 0, 0});
                for (i32 r0 = kb + nb; r0 < w.f; r0 += SOLVE_ROWS) {
                    const bool first = (r0 == kb + nb);
                    if ((round == 0) != first) continue;
                    S.fwd_update_tasks.push_back(SolveTask{s, kb, nb, r0, 0, (first && next_nb > 0) ? next_nb : 0, 0, 0});
                }
            }
            push_launch(S.fwd_launches, Scope{g, 0}, LK_FWD_DIAG, f_diag, (i64)S.fwd_diag_tasks.size() - f_diag);
            push_launch(S.fwd_launches, Scope{g, 0}, LK_FWD_UPDATE, f_upd, (i64)S.fwd_update_tasks.size() - f_upd);
        }
    }
    // Backward solve of one level.  Column-oriented: launch 0 of a level removes the rows below the pivot block (known from the
    // ancestors) from every column block of every front and solves each front's last block; launch
    // b >= 1 removes the block solved by launch b-1 from the column blocks before it and solves the
    // next one.  SolveTask fields here: k0/nb = target column block, row0/slot = first source row
    // and number of source rows, nslot != 0 = also solve the diagonal block k0.
    void bwd_level(int g, i32 d) {
        const i32 t0 = S.level_ptr[d], t1 = S.level_ptr[d + 1];
        const auto [small_first, small_count] = small_front_list(g, t0, t1, S.bwd_small_tasks);
        const i32 max_ns = max_ns_not_small(g, t0, t1);
        if (S.sweep) {
            // hand-out order: distance of the column block from the END of its front first (a block waits for the
            // later blocks of its own front only), front second
            const i64 first = (i64)S.bwd_sweep_tasks.size();
            const i32 nblk64 = (max_ns + SWEEP_NB - 1) / SWEEP_NB;
            for (i32 dd = 0; dd < nblk64; ++dd)
                for (i32 t = t0; t < t1; ++t) {
                    const i32 s = S.level_fronts[t];
                    if (!in_scope(s, g) || is_small(s)) continue;
                    const FrontDesc &w = S.fronts[s];
                    const i32 my_nblk = (w.ns + SWEEP_NB - 1) / SWEEP_NB;
                    if (dd >= my_nblk) continue;
                    const i32 kb = my_nblk - 1 - dd;
                    S.bwd_sweep_tasks.push_back(SolveTask{s, kb * SWEEP_NB, std::min(SWEEP_NB, w.ns - kb * SWEEP_NB), w.ns, w.f - w.ns, dd, 0, 0});
                }
            small_and_sweep_launches(g, false, small_first, small_count, first);
            return;
        }
        push_launch(S.bwd_launches, Scope{g, 0}, LK_BWD_SMALL, small_first, small_count);      // (in stream order)
        const i32 nblk = (max_ns + SOLVE_NB - 1) / SOLVE_NB;
        for (i32 b = 0; b < nblk; ++b) {
            const i64 f_upd = (i64)S.bwd_update_tasks.size();
            // round 0: the workgroups that also solve a diagonal block (critical path) start first
            for (int round = 0; round < 2; ++round)
            for (i32 t = t0; t < t1; ++t) {
                const i32 s = S.level_fronts[t];
                if (!in_scope(s, g) || is_small(s)) continue;
                const FrontDesc &w = S.fronts[s];
                const i32 my_nblk = (w.ns + SOLVE_NB - 1) / SOLVE_NB;
                if (b >= my_nblk) continue;
                const i32 ksrc = my_nblk - b;                       // source block (== my_nblk: rows below the pivot block)
                const i32 row0 = (b == 0) ? w.ns : ksrc * SOLVE_NB;
                const i32 nrows = (b == 0) ? (w.f - w.ns) : std::min(SOLVE_NB, w.ns - row0);
                for (i32 J = ksrc - 1; J >= 0; --J) {
                    const bool diag = (J == ksrc - 1);
                    if ((round == 0) != diag) continue;
                    if (!diag && nrows == 0) continue;
                    S.bwd_update_tasks.push_back(SolveTask{s, J * SOLVE_NB, std::min(SOLVE_NB, w.ns - J * SOLVE_NB), row0, nrows, diag ? 1 : 0, 0, 0});
                }
            }
            push_launch(S.bwd_launches, Scope{g, 0}, LK_BWD_UPDATE, f_upd, (i64)S.bwd_update_tasks.size() - f_upd);
        }
    }
};

}  // namespace

void build_schedule(Symbolic &S) {
    PhaseTimer spt; spt.mark("schedule: prologue");
    ScheduleBuilder B(S);
    B.singles_and_upper_fronts();
    B.zero_fill_lists();
    spt.mark("schedule: factor");
    for (int g = 0; g < S.ngroups; ++g)
        for (i32 d = S.nlevels - 1; d >= 1; --d) B.factor_level(g, d);
    if (S.nlevels > 0) B.factor_level(-1, 0);
    B.make_slots_absolute();
    spt.mark("schedule: fwd");
    // forward solve: deepest level first
    B.solve_flags();
    // One solve schedule for all stream groups (round 5, default; TLPK_SOLVE_ONE_GROUP=0 restores one schedule per group).  The stream groups exist
    // for the factorisation, whose launches leave tails that a second group fills.  The solve's big launches are the persistent, ticketed sweeps:
    // one of them fills the chip, and a second group's leaf-level launches then crawl beside the first group's sweep -- in the paired solve the two
    // groups' forward sweeps ran one after the other (629 + 650 us, profiles/r04_solve_timeline.txt).  With scope -1 a level's launch holds the
    // fronts of every group and runs on the main stream; per-item arithmetic is unchanged (bit-identical results).
    const bool solve_one_group = S.ngroups >= 2 && B.K.solve_one_group;
    S.solve_single_stream = solve_one_group || S.ngroups <= 1;
    const int g0 = solve_one_group ? -1 : 0, g1 = solve_one_group ? 0 : S.ngroups;      // scopes [g0, g1) serve the levels below depth 0
    for (int g = g0; g < g1; ++g)
        for (i32 d = S.nlevels - 1; d >= 1; --d) B.fwd_level(g, d);
    if (S.nlevels > 0) B.fwd_level(-1, 0);
    spt.mark("schedule: bwd");
    // backward solve: root level first
    if (S.nlevels > 0) B.bwd_level(-1, 0);
    for (int g = g0; g < g1; ++g)
        for (i32 d = 1; d < S.nlevels; ++d) B.bwd_level(g, d);
    spt.mark(nullptr);
}

}  // namespace tlpk
