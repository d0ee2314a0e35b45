// schedule.hpp -- what the analysis (symbolic.cpp) and the schedule builder (schedule.cpp) share: the extend-add ranges of a parent front,
// the phase timer of TLPK_TIMING, and build_schedule itself.  Internal to the host analyse phase.
#pragma once
#include "tlpk_host.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>

namespace tlpk {

// Extend-add ranges of a parent front (one workgroup each): ea_cols(p) columns wide, counted from 0 inside the pivot
// columns [0, ns) and from ns inside the update-matrix columns [ns, f).  Boundary k of ea_nbounds(p):
//   k < npan: k * cols ; k == npan: ns ; k > npan: ns + (k - npan) * cols, the last one being f.
inline i32 ea_cols_big() {              // TLPK_EA_COLS (tuning knob, 4 .. EA_COLS): parent columns per extend-add workgroup of the big fronts; read once per process
    static const i32 v = [] { const char *e = std::getenv("TLPK_EA_COLS"); const int c = e ? std::atoi(e) : EA_COLS; return (i32)std::max(4, std::min(c, EA_COLS)); }();
    return v;
}
inline i32 ea_cols(const FrontDesc &p, bool fa) { return fa ? FA_CW : ((p.f >= 2048) ? ea_cols_big() : 4); }     // small fronts: more, narrower workgroups
inline i32 ea_npan(const FrontDesc &p, bool fa) { const i32 c = ea_cols(p, fa); return (p.ns + c - 1) / c; }
inline i32 ea_nbounds(const FrontDesc &p, bool fa) { const i32 c = ea_cols(p, fa); return ea_npan(p, fa) + (p.f - p.ns + c - 1) / c + 1; }
inline i32 ea_bound(const FrontDesc &p, bool fa, i32 k) {
    const i32 c = ea_cols(p, fa), npan = ea_npan(p, fa);
    return (k < npan) ? k * c : std::min(p.f, p.ns + (k - npan) * c);
}

// TLPK_TIMING=1: wall time of the analyse phases on stderr
struct PhaseTimer {
    bool on; std::chrono::steady_clock::time_point t0; const char *name = nullptr;
    PhaseTimer() : on(std::getenv("TLPK_TIMING") != nullptr), t0(std::chrono::steady_clock::now()) {}
    void mark(const char *next) {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        if (name) std::fprintf(stderr, "[tlpk analyse] %-28s %8.1f ms\n", name, std::chrono::duration<double, std::milli>(t1 - t0).count());
        name = next; t0 = t1;
    }
};

// schedule.cpp: every task list and launch list a handle replays (zero-fill, assembly, blocked factorisation, LK_CHAIN items, the two sweeps), from the
// front structures, ownership and storage offsets analyse_rank / analyse_dense_matrix have filled in.  Sets S.error on an inconsistent chain schedule.
void build_schedule(Symbolic &S);

}  // namespace tlpk
