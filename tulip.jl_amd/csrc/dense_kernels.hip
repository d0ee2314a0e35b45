// dense_kernels.hip -- kernels of the dense-matrix handles (tlpk_create_dense): the counterpart of the reference's dense backend
// (/root/reference/src/KKT/Dense/lapack.jl:52-119: scale, A D A', cholesky!; two GEMVs around two triangular solves).
//
// A is a column-major m x n array on the device, leading dimension lda = m rounded up to 16 doubles (columns start on 128-byte
// lines), padding rows zero, read-only for the life of the handle.
//   k_dense_syrk         lower triangle of S = A diag(D) A' + diag(regD) on the fp64 matrix cores, written straight into the packed
//                        panel of the handle's one front (tlpk_host.hpp: pk_off) -- no scaled copy of A, no m x m intermediate, no
//                        zero-fill: every stored entry of the panel is written.  The two operands of a tile are row ranges of A, K runs
//                        along its columns: the shape of the panel update (kernels.hip: update_tile) with a + sign and a weight per K.
//   k_dense_syrk_reduce  few tiles (small m): K = n is cut into parts, one workgroup each; the raw partial tiles are summed in part order
//   k_dense_gemv_n       xi_p + A (D .* xi_d)        (lapack.jl:105-106), one or two right-hand sides in one pass over A
//   k_dense_gemv_t       D .* (A' dy - xi_d)         (lapack.jl:113-116), likewise
// All sums have a fixed order (no floating-point atomics): two runs on the same input give the same bits.
#include <hip/hip_runtime.h>

#include "tlpk_device.hpp"

namespace tlpk {

typedef double v4f64 __attribute__((ext_vector_type(4)));

constexpr int DS_KT = 16;                  // K depth staged per LDS round
constexpr int DS_LD = TILE + 16;           // LDS row stride (doubles), == 16 mod 32: conflict-free b64 reads
constexpr int DS_RED = 8;                  // workgroups per tile in k_dense_syrk_reduce (TILE / DS_RED columns each)

// tile t of the lower triangle, row-major over (ti, tj <= ti)
__device__ __forceinline__ void syrk_tile(const unsigned t, i32 &ti, i32 &tj) {
    i32 r = (i32)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((unsigned)(r + 1) * (unsigned)(r + 2) / 2 <= t) ++r;
    while ((unsigned)r * (unsigned)(r + 1) / 2 > t) --r;
    ti = r; tj = (i32)(t - (unsigned)r * (unsigned)(r + 1) / 2);
}

// one entry of the tile -> the packed panel: the lower triangle gets its value (+ regD on the diagonal; exactly 0 on the padding rows
// m .. lda - 1), the part of a 64 x 64 diagonal block above the diagonal gets 0 (the diagonal-block kernels load whole blocks), anything
// above the first row of the column's 64-column slice has no storage
__device__ __forceinline__ void syrk_store(double *__restrict__ P, const i32 plda, const i32 m, const i32 row, const i32 col, const double v,
                                           const double *__restrict__ regD) {
    if (row >= plda || col >= m) return;
    if (row >= col) P[pk_off(plda, col) + row] = (row < m) ? ((row == col) ? v + regD[row] : v) : 0.0;
    else if (row >= ((col >> 6) << 6)) P[pk_off(plda, col) + row] = 0.0;
}

struct SyrkArgs {
    const double *A; i64 lda; i32 m; i64 n;
    i64 kc; i32 split;                     // K parts: part p = columns [p kc, min(n, (p + 1) kc)), kc a multiple of DS_KT
    const double *D, *regD;
    double *P; i32 plda;                   // the front's packed panel and its leading dimension
    double *spart;                         // split > 1: raw partial tiles, slot = tile * split + part
};

// 256 threads = 2 x 2 waves, a 64 x 64 sub-tile each (16 accumulator blocks of v_mfma_f64_16x16x4_f64); operands staged as update_tile does:
// thread (sr = tid & 127, sk0 = tid >> 7) carries row sr of both operand tiles for the K columns sk0, sk0 + 2, ... of a slab; the slab after the
// one being multiplied travels global -> registers during the MFMA block and registers -> LDS behind it.  D is applied to the COLUMN-tile operand
// while it is staged (the K column of a staging load is wave-uniform: D[k] is a scalar load).
__global__ __launch_bounds__(256, 2) void k_dense_syrk(const SyrkArgs g) {
    __shared__ __attribute__((aligned(16))) double As[2][DS_KT * DS_LD];   // As[.][k][r] = A[i0 + r, k]          (row tile)
    __shared__ __attribute__((aligned(16))) double Bs[2][DS_KT * DS_LD];   // Bs[.][k][r] = A[j0 + r, k] D[k]     (column tile)
    i32 ti, tj;
    syrk_tile(blockIdx.x, ti, tj);
    const i32 i0 = ti * TILE, j0 = tj * TILE;
    const i64 k_lo = (i64)blockIdx.y * g.kc, k_hi = min(g.n, k_lo + g.kc);
    const i64 kw = max((i64)0, k_hi - k_lo);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1, lr = lane & 15, lk = lane >> 4;
    const bool any = !(ti == tj && wr == 0 && wc == 1);            // the diagonal tile's upper-right quarter is never stored (wave-uniform)
    const int sr = tid & 127;
    const int sk0 = __builtin_amdgcn_readfirstlane(tid >> 7);
    // rows beyond the last stored row are clamped: they feed entries the epilogue never stores
    const i64 ra = min((i64)i0 + sr, g.lda - 1), rb = min((i64)j0 + sr, g.lda - 1);
    constexpr int NLD = DS_KT / 2;
    double pa[NLD], pb[NLD];
    v4f64 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (v4f64){0.0, 0.0, 0.0, 0.0};

    auto load_slab = [&](const i64 kk) {
        if (kk + DS_KT <= kw) {
#pragma unroll
            for (int it = 0; it < NLD; ++it) {
                const i64 k = k_lo + kk + sk0 + 2 * it;
                const double *Ak = g.A + k * g.lda;
                pa[it] = Ak[ra];
                pb[it] = Ak[rb] * g.D[k];
            }
        } else {
#pragma unroll
            for (int it = 0; it < NLD; ++it) {
                const bool kok = kk + sk0 + 2 * it < kw;
                const i64 k = k_lo + min(kk + sk0 + 2 * it, kw - 1);
                const double *Ak = g.A + k * g.lda;
                pa[it] = kok ? Ak[ra] : 0.0;
                pb[it] = kok ? Ak[rb] * g.D[k] : 0.0;
            }
        }
    };
    auto store_slab = [&](const int buf) {
#pragma unroll
        for (int it = 0; it < NLD; ++it) {
            As[buf][(sk0 + 2 * it) * DS_LD + sr] = pa[it];
            Bs[buf][(sk0 + 2 * it) * DS_LD + sr] = pb[it];
        }
    };
    if (kw > 0) {
        load_slab(0);
        store_slab(0);
        __syncthreads();
        int cur = 0;
        for (i64 kk = 0; kk < kw; kk += DS_KT) {
            const bool more = kk + DS_KT < kw;
            if (more) load_slab(kk + DS_KT);                        // in flight during the MFMA block
            if (any) {
                const double *At = As[cur] + wr * 64 + lr + lk * DS_LD;
                const double *Bt = Bs[cur] + wc * 64 + lr + lk * DS_LD;
#pragma unroll
                for (int k4 = 0; k4 < DS_KT; k4 += 4) {
                    double av[4], bv[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) av[a] = Bt[k4 * DS_LD + a * 16];      // column-tile rows
#pragma unroll
                    for (int b = 0; b < 4; ++b) bv[b] = At[k4 * DS_LD + b * 16];      // row-tile rows
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
                }
            }
            if (more) store_slab(cur ^ 1);
            __syncthreads();
            cur ^= 1;
        }
    }
    if (!any) return;
    // acc[a][b][q] = S[i0 + 64 wr + 16 b + lr, j0 + 64 wc + 16 a + lk + 4 q]: 16 consecutive rows per (a, b, q) and lk -- coalesced column-major stores
    if (g.split > 1) {
        double *Sp = g.spart + ((i64)blockIdx.x * g.split + blockIdx.y) * (TILE * TILE);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int q = 0; q < 4; ++q) Sp[(wr * 64 + b * 16 + lr) + (wc * 64 + a * 16 + lk + 4 * q) * TILE] = acc[a][b][q];
        return;
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                syrk_store(g.P, g.plda, g.m, i0 + wr * 64 + b * 16 + lr, j0 + wc * 64 + a * 16 + lk + 4 * q, acc[a][b][q], g.regD);
}

// the parts of one tile, summed in part order (k_update_reduce is the model); DS_RED workgroups per tile
__global__ __launch_bounds__(256) void k_dense_syrk_reduce(const SyrkArgs g) {
    const unsigned t = blockIdx.x / DS_RED, part = blockIdx.x % DS_RED;
    i32 ti, tj;
    syrk_tile(t, ti, tj);
    const double *Sp = g.spart + (i64)t * g.split * (TILE * TILE);
    constexpr int PER = TILE * TILE / DS_RED;
    for (int e = (int)part * PER + (int)threadIdx.x; e < ((int)part + 1) * PER; e += 256) {
        const i32 row = ti * TILE + (e & (TILE - 1)), col = tj * TILE + (e >> 7);
        double sum = 0.0;
        if (row >= col && row < g.m && col < g.m) {
            sum = Sp[e];
            for (i32 sp = 1; sp < g.split; ++sp) sum += Sp[(i64)sp * (TILE * TILE) + e];
        }
        syrk_store(g.P, g.plda, g.m, row, col, sum, g.regD);
    }
}

// ------------------------------------------------------------------------------------------
// GEMV, no transpose: partial[chunk][i] = sum_{j in chunk} A[i, j] w[j], w = D .* x (D != nullptr) or x.  A thread owns two consecutive rows
// (16-byte loads, a wave reads 1 KB of a column), a workgroup DGEMV_ROWS rows x one chunk of columns; k_dense_gemv_n_sum adds the chunks in
// chunk order (+ the vector `add`).  NR = 2: both right-hand sides of a pair from ONE pass over A, each with the arithmetic of NR = 1.
// ------------------------------------------------------------------------------------------
struct GemvArgs {
    const double *A; i64 lda, m, n;
    i64 cw, chunks;                        // columns per chunk, number of chunks
    const double *D;                       // nullptr: no scaling
    const double *x[2];                    // gemv_n: the vectors multiplied (length n); gemv_t: y (length m)
    const double *add[2];                  // gemv_n: added to the sums (length m) or nullptr; gemv_t: xi_d (subtracted before the scaling) or nullptr
    double *out[2];
    double *part;                          // gemv_n: [NR][chunks][lda] partial sums
};
template <int NR>
__global__ __launch_bounds__(256) void k_dense_gemv_n(const GemvArgs g) {
    const i64 row = ((i64)blockIdx.x * 256 + threadIdx.x) * 2;
    if (row >= g.lda) return;                                   // (lda is even: row + 1 < lda)
    const i64 j0 = (i64)blockIdx.y * g.cw, j1 = min(g.n, j0 + g.cw);
    double s[NR][2];
#pragma unroll
    for (int r = 0; r < NR; ++r) s[r][0] = s[r][1] = 0.0;
    const double *Ac = g.A + row;
#pragma unroll 4
    for (i64 j = j0; j < j1; ++j) {
        const double2 a = *reinterpret_cast<const double2 *>(Ac + j * g.lda);
        const double d = g.D ? g.D[j] : 1.0;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const double w = g.D ? d * g.x[r][j] : g.x[r][j];
            s[r][0] = fma(a.x, w, s[r][0]);
            s[r][1] = fma(a.y, w, s[r][1]);
        }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r)
        *reinterpret_cast<double2 *>(g.part + ((i64)r * g.chunks + blockIdx.y) * g.lda + row) = make_double2(s[r][0], s[r][1]);
}
__global__ __launch_bounds__(256) void k_dense_gemv_n_sum(const GemvArgs g) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const int r = blockIdx.y;                                   // (grid y = right-hand side of a pair)
    if (i >= g.m) return;
    const double *p = g.part + (i64)r * g.chunks * g.lda + i;
    double s = 0.0;
    for (i64 c = 0; c < g.chunks; ++c) s += p[c * g.lda];
    g.out[r][i] = g.add[r] ? g.add[r][i] + s : s;
}

// GEMV, transpose: out[j] = D[j] (A[:, j]' y - xi_d[j])  (D == nullptr: A[:, j]' y).  One wave per column: lane l takes the row pairs l, l + 64, ...
// (16-byte loads of a contiguous column), then a fixed butterfly over the 64 lanes.
template <int NR>
__global__ __launch_bounds__(256) void k_dense_gemv_t(const GemvArgs g) {
    const int lane = threadIdx.x & 63;
    const i64 j = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= g.n) return;                                       // (wave-uniform)
    const double2 *col = reinterpret_cast<const double2 *>(g.A + j * g.lda);
    const i64 npair = g.lda / 2;
    double s[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) s[r] = 0.0;
#pragma unroll 4
    for (i64 p = lane; p < npair; p += 64) {
        const double2 a = col[p];                               // padding rows of A are zero; y is not read beyond m
        const bool ok0 = 2 * p < g.m, ok1 = 2 * p + 1 < g.m;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const double y0 = ok0 ? g.x[r][2 * p] : 0.0, y1 = ok1 ? g.x[r][2 * p + 1] : 0.0;
            s[r] = fma(a.x, y0, s[r]);
            s[r] = fma(a.y, y1, s[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s[r] += __shfl_xor(s[r], off, 64);
        if (lane == 0) g.out[r][j] = g.D ? g.D[j] * (s[r] - g.add[r][j]) : s[r];
    }
}

// ------------------------------------------------------------------------------------------
static inline unsigned nblk(i64 n, int b) { return (unsigned)((n + b - 1) / b); }

void launch_dense_syrk(hipStream_t st, const DevArrays &a, const double *D, const double *regD, double *P, i32 plda) {
    const i64 T = (a.m + TILE - 1) / TILE, ntiles = T * (T + 1) / 2;
    const SyrkArgs g{a.dA, a.dlda, (i32)a.m, a.n, a.syrk_kc, a.syrk_split, D, regD, P, plda, a.ctx.spart};
    hipLaunchKernelGGL(k_dense_syrk, dim3((unsigned)ntiles, (unsigned)a.syrk_split), dim3(256), 0, st, g);
    if (a.syrk_split > 1) hipLaunchKernelGGL(k_dense_syrk_reduce, dim3((unsigned)(ntiles * DS_RED)), dim3(256), 0, st, g);
}

void launch_dense_gemv_n(hipStream_t st, const DevArrays &a, const double *D, const double *const *x, const double *const *add, double *const *out, int nrhs) {
    if (a.m <= 0) return;
    GemvArgs g{a.dA, a.dlda, a.m, a.n, a.gemv_cw, a.gemv_chunks, D, {x[0], x[nrhs - 1]}, {add[0], add[nrhs - 1]}, {out[0], out[nrhs - 1]}, a.gemv_part};
    if (a.n <= 0) g.chunks = 0;                                 // no columns: the sums are empty
    else {
        const dim3 grid(nblk(a.dlda, DGEMV_ROWS), (unsigned)a.gemv_chunks);
        if (nrhs == 2) hipLaunchKernelGGL(k_dense_gemv_n<2>, grid, dim3(256), 0, st, g);
        else hipLaunchKernelGGL(k_dense_gemv_n<1>, grid, dim3(256), 0, st, g);
    }
    hipLaunchKernelGGL(k_dense_gemv_n_sum, dim3(nblk(a.m, 256), (unsigned)nrhs), dim3(256), 0, st, g);
}

void launch_dense_gemv_t(hipStream_t st, const DevArrays &a, const double *D, const double *const *y, const double *const *xi_d, double *const *out, int nrhs) {
    if (a.n <= 0) return;
    const GemvArgs g{a.dA, a.dlda, a.m, a.n, 0, 0, D, {y[0], y[nrhs - 1]}, {xi_d[0], xi_d[nrhs - 1]}, {out[0], out[nrhs - 1]}, nullptr};
    if (nrhs == 2) hipLaunchKernelGGL(k_dense_gemv_t<2>, dim3(nblk(a.n, 4)), dim3(256), 0, st, g);
    else hipLaunchKernelGGL(k_dense_gemv_t<1>, dim3(nblk(a.n, 4)), dim3(256), 0, st, g);
}

}  // namespace tlpk
