// krylov_spmv.hpp -- the sparse gather of the matrix-free kernels (krylov_kernels.hip, krylov_k2_kernels.hip, krylov_sqd_kernels.hip): one sum per row of the
// row-wise copy of A or per column of its CSC copy.  Rows and columns of an LP hold a handful of entries: a short row gets 8 lanes, a short column 4.  One with
// more than CG_LONG entries (a linking row, a dense column) is listed at create and gets a whole workgroup.  A kernel passes two callables: term(q), the
// addend of entry q, and done(i, s), what ONE lane does with the finished sum s of item i (store it, add to the workgroup's partial sum).  The order of the
// additions is fixed by the lane count and the trees below and is part of the bit-reproducibility contract of krylov_reduce.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "krylov_reduce.hpp"
#include "tlpk_device.hpp"

namespace tlpk {

// The short items of [0, n_items): LANES lanes each, handed out round by round to `parts` workgroups of T threads, of which this is number `part` (every
// wave makes the same number of rounds; a grid of ceil(n_items LANES / T) workgroups makes one).  An item longer than CG_LONG is left to walk_long.
// NR right-hand sides share the walk: entry(q) reads the index and the value of entry q ONCE, term(e, r) is its addend for right-hand side r, and
// done(i, s, r) takes the finished sum.  Every sum has the lanes and the shuffle tree of the single walk; a right-hand side that is not on is neither
// read nor written (on[r] is the same in every lane of the grid).
template <int T, int LANES, int NR, class Entry, class Term, class Done>
__device__ __forceinline__ void walk_short(i64 n_items, const i64 *__restrict__ ptr, unsigned part, unsigned parts, const bool (&on)[NR], Entry entry, Term term,
                                           Done done) {
    const int lane = threadIdx.x & (LANES - 1);
    for (i64 base = 0; base < n_items; base += (i64)parts * T / LANES) {
        const i64 i = base + ((i64)part * T + threadIdx.x) / LANES;
        const bool live = i < n_items;
        const i64 q0 = live ? ptr[i] : 0, q1 = live ? ptr[i + 1] : 0;
        const bool mine = live && q1 - q0 <= CG_LONG;
        double s[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) s[r] = 0.0;
        if (mine) for (i64 q = q0 + lane; q < q1; q += LANES) {
            const auto e = entry(q);
#pragma unroll
            for (int r = 0; r < NR; ++r) if (on[r]) s[r] += term(e, r);
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            if (!on[r]) continue;
#pragma unroll
            for (int off = LANES / 2; off > 0; off >>= 1) s[r] += __shfl_down(s[r], off, LANES);
            if (mine && lane == 0) done(i, s[r], r);
        }
    }
}
// one right-hand side, the addend straight from the entry's number (the kernels of an update)
template <int T, int LANES, class Term, class Done>
__device__ __forceinline__ void walk_short(i64 n_items, const i64 *__restrict__ ptr, unsigned part, unsigned parts, Term term, Done done) {
    const bool on[1] = {true};
    walk_short<T, LANES, 1>(n_items, ptr, part, parts, on, [](i64 q) { return q; }, [&](i64 q, int) { return term(q); }, [&](i64 i, double s, int) { done(i, s); });
}

// The long items list[first], list[first + stride], ...: the whole workgroup (T threads) strides over one item at a time; sh holds T / 64 doubles.  A kernel
// that gives every long item a workgroup of its own passes stride = n_list.  NR, entry, term, done, on: as walk_short.
template <int T, int NR, class Entry, class Term, class Done>
__device__ __forceinline__ void walk_long(const i32 *__restrict__ list, i64 n_list, i64 first, i64 stride, const i64 *__restrict__ ptr, double *sh,
                                          const bool (&on)[NR], Entry entry, Term term, Done done) {
    for (i64 k = first; k < n_list; k += stride) {
        const i64 i = list[k];
        double s[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) s[r] = 0.0;
        for (i64 q = ptr[i] + threadIdx.x; q < ptr[i + 1]; q += T) {
            const auto e = entry(q);
#pragma unroll
            for (int r = 0; r < NR; ++r) if (on[r]) s[r] += term(e, r);
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            if (!on[r]) continue;
            s[r] = cg_block_sum<T>(s[r], sh);
            if (threadIdx.x == 0) done(i, s[r], r);
        }
    }
}
template <int T, class Term, class Done>
__device__ __forceinline__ void walk_long(const i32 *__restrict__ list, i64 n_list, i64 first, i64 stride, const i64 *__restrict__ ptr, double *sh, Term term,
                                          Done done) {
    const bool on[1] = {true};
    walk_long<T, 1>(list, n_list, first, stride, ptr, sh, on, [](i64 q) { return q; }, [&](i64 q, int) { return term(q); }, [&](i64 i, double s, int) { done(i, s); });
}

// an entry of A as the gathers read it: its value and the index of the other dimension
struct SpEntry { double a; i32 i; };

inline unsigned nblk(i64 n, int b) { return (unsigned)((n + b - 1) / b); }

}  // namespace tlpk
