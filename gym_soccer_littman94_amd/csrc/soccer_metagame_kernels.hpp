// soccer_metagame_kernels.hpp — the maximin mixtures of n_a x n_b zero-sum matrix games (soccer_solve_meta_games; the
// definition is in include/soccer_hip.h, "the meta-game").  Included by soccer_metagame.hip only.
//
// One set of block-level functions states the arithmetic once: meta_setup (the saddle-point test and the tableau),
// meta_select (Dantzig's column, the ratio test with the shadow column's tie-break, the scaled pivot row and the column of factors),
// meta_extract and meta_finish (the strategies and the bracket).  They take plain pointers, so the same code runs
//   * on a tableau in LDS: meta_lds_kernel, a workgroup per game, the whole solve in one launch;
//   * on a tableau in HBM: meta_setup_kernel, then per pivot meta_select_kernel (a workgroup per game) and
//     meta_update_kernel (a 2-D grid of tiles x games), then meta_finish_kernel; ordering is the stream's.
// Every reduction orders (value, index) pairs, so no bit depends on how the work is spread over threads; every entry of the
// tableau is updated by the one expression T - f * p (two roundings: the units are compiled with -ffp-contract=off).
//
// The row stride is odd: the ratio test and the column of factors read the pivot column down a stride, and with an even
// stride of doubles those 8-byte reads of a wave fall on few LDS banks (64 banks of 4 bytes: stride 64 is a 32-way conflict).
#pragma once
#include <climits>

#include "soccer_plan_io.hpp"

namespace soccer {

constexpr int kMetaBlock = 256;
constexpr int kMetaWaves = kMetaBlock / 64;
constexpr int kMetaTileRows = 16;                 // meta_update_kernel: a block owns 16 rows x 256 columns
constexpr double kMetaTol = 1e-12;                // entries of the scaled tableau are O(1)

struct MetaRed { double v[kMetaWaves]; double w[kMetaWaves]; int32_t i[kMetaWaves]; int32_t pad[12]; };   // the cross-wave step
static_assert(sizeof(MetaRed) == 128, "the fit rule of the LDS path counts 128 bytes");

__host__ __device__ inline int meta_stride(int n_a, int n_b) { return (n_a + n_b + 2) | 1; }
// what meta_lds_kernel needs: the reduction words, the tableau, the pivot row, the factors, the basis
__host__ __device__ inline size_t meta_lds_bytes(int n_a, int n_b) {
    return 128 + 8 * ((size_t)(n_a + 2) * meta_stride(n_a, n_b) + n_a + 1) + 4 * (size_t)n_a;
}

// does (v, w, i) come before (bv, bw, bi)?  the smaller v (MAX: the larger), then the smaller w, then the lower index
template <bool MAX>
__device__ __forceinline__ bool meta_before(double v, double w, int i, double bv, double bw, int bi) {
    return (MAX ? v > bv : v < bv) || (v == bv && (w < bw || (w == bw && i < bi)));
}
template <bool MAX>
__device__ __forceinline__ bool meta_before(double v, int i, double bv, int bi) { return meta_before<MAX>(v, 0.0, i, bv, 0.0, bi); }

// the first (v, w, i) of the block in that order, returned to every thread.  A thread with nothing passes (+-inf, 0, INT_MAX).
template <bool MAX>
__device__ __forceinline__ void meta_block_arg(double& v, double& w, int& i, MetaRed* red) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const double ov = __shfl_down(v, o, 64), ow = __shfl_down(w, o, 64);
        const int oi = __shfl_down(i, o, 64);
        if (meta_before<MAX>(ov, ow, oi, v, w, i)) { v = ov; w = ow; i = oi; }
    }
    if ((threadIdx.x & 63u) == 0) { red->v[threadIdx.x >> 6] = v; red->w[threadIdx.x >> 6] = w; red->i[threadIdx.x >> 6] = i; }
    __syncthreads();
    v = red->v[0]; w = red->w[0]; i = red->i[0];
#pragma unroll
    for (int k = 1; k < kMetaWaves; ++k) {
        const double ov = red->v[k], ow = red->w[k];
        const int oi = red->i[k];
        if (meta_before<MAX>(ov, ow, oi, v, w, i)) { v = ov; w = ow; i = oi; }
    }
    __syncthreads();
}
template <bool MAX>
__device__ __forceinline__ void meta_block_arg(double& v, int& i, MetaRed* red) { double w = 0.0; meta_block_arg<MAX>(v, w, i, red); }

// the saddle-point test and, without one, the tableau and the slack basis.  true: a saddle point at (istar, jstar).
__device__ __forceinline__ bool meta_setup(const double* A, int n_a, int n_b, int stride, double* T, int32_t* basis, MetaRed* red,
                                           int& istar, int& jstar, double& amax) {
    const int tid = (int)threadIdx.x;
    const double inf = __builtin_huge_val();
    double v_hi = -inf, v_lo = inf; int i_hi = INT_MAX, i_lo = INT_MAX;
    for (int i = tid; i < n_a; i += kMetaBlock) {                       // a row's minimum
        const double* a = A + (size_t)i * n_b;
        double m = a[0];
        for (int j = 1; j < n_b; ++j) m = a[j] < m ? a[j] : m;
        if (meta_before<true>(m, i, v_hi, i_hi)) { v_hi = m; i_hi = i; }
        if (meta_before<false>(m, i, v_lo, i_lo)) { v_lo = m; i_lo = i; }
    }
    meta_block_arg<true>(v_hi, i_hi, red);
    meta_block_arg<false>(v_lo, i_lo, red);
    const double maxmin = v_hi, lo_a = v_lo;
    istar = i_hi;
    v_hi = -inf; v_lo = inf; i_hi = INT_MAX; i_lo = INT_MAX;
    for (int j = tid; j < n_b; j += kMetaBlock) {                       // a column's maximum
        double m = A[j];
        for (int i = 1; i < n_a; ++i) { const double a = A[(size_t)i * n_b + j]; m = a > m ? a : m; }
        if (meta_before<false>(m, j, v_lo, i_lo)) { v_lo = m; i_lo = j; }
        if (meta_before<true>(m, j, v_hi, i_hi)) { v_hi = m; i_hi = j; }
    }
    meta_block_arg<false>(v_lo, i_lo, red);
    meta_block_arg<true>(v_hi, i_hi, red);
    const double minmax = v_lo, hi_a = v_hi;
    jstar = i_lo;
    amax = hi_a > -lo_a ? hi_a : -lo_a;
    if (maxmin == minmax) return true;
    const double range = hi_a - lo_a;
    const int rows = n_a + 1, R = n_a + n_b;
    int i = 0, j = tid;
    while (j >= stride) { j -= stride; ++i; }
    while (i < rows) {
        double t = 0.0;
        if (i < n_a) {
            if (j < n_b) t = (A[(size_t)i * n_b + j] - lo_a) / range + 1.0;
            else if (j < R) t = j - n_b == i ? 1.0 : 0.0;
            else if (j == R) t = 1.0;
            else if (j == R + 1) t = 1.0 + (double)(i + 1) * 0x1p-26;   // the shadow right-hand side
        } else if (j < n_b) t = -1.0;
        T[(size_t)i * stride + j] = t;
        j += kMetaBlock;
        while (j >= stride) { j -= stride; ++i; }
    }
    for (int k = tid; k < n_a; k += kMetaBlock) basis[k] = n_b + k;
    __syncthreads();
    return false;
}

// one pivot's choice.  0: column c and row r are chosen, prow holds the scaled pivot row and fcol the pivot column;
// 1: the game is finished; 3: stopped (the cap, or no row passes the ratio test)
__device__ __forceinline__ int meta_select(const double* T, int n_a, int n_b, int stride, int pivots, int max_pivots,
                                           double* prow, double* fcol, MetaRed* red, int& c, int& r) {
    const int tid = (int)threadIdx.x;
    const double inf = __builtin_huge_val();
    const double* obj = T + (size_t)n_a * stride;
    double v = inf; int k = INT_MAX;
    for (int j = tid; j < n_a + n_b; j += kMetaBlock) {
        const double t = obj[j];
        if (meta_before<false>(t, j, v, k)) { v = t; k = j; }
    }
    meta_block_arg<false>(v, k, red);
    c = k;
    if (!(v < -kMetaTol)) return 1;
    if (pivots == max_pivots) return 3;
    const int R = n_a + n_b, S = R + 1;
    double w = 0.0;
    v = inf; k = INT_MAX;
    for (int i = tid; i < n_a; i += kMetaBlock) {
        const double p = T[(size_t)i * stride + c];
        if (p > kMetaTol) {
            const double q = T[(size_t)i * stride + R] / p, qs = T[(size_t)i * stride + S] / p;
            if (meta_before<false>(q, qs, i, v, w, k)) { v = q; w = qs; k = i; }
        }
    }
    meta_block_arg<false>(v, w, k, red);
    if (k == INT_MAX) return 3;
    r = k;
    const double* row = T + (size_t)r * stride;
    const double piv = row[c];
    for (int j = tid; j < stride; j += kMetaBlock) prow[j] = j == c ? 1.0 : row[j] / piv;
    for (int i = tid; i <= n_a; i += kMetaBlock) fcol[i] = T[(size_t)i * stride + c];
    __syncthreads();
    return 0;
}

// one entry after the pivot at (r, c): row r is the scaled row, column c is zero elsewhere, no row is skipped
__device__ __forceinline__ double meta_entry(double t, double f, double p, bool pivot_row, bool pivot_col) {
    return pivot_row ? p : (pivot_col ? 0.0 : t - f * p);
}

// the strategies of the basis, clipped at 0, not yet normalised: ys from the true right-hand side, xs from the objective row
__device__ __forceinline__ void meta_extract(const double* T, const int32_t* basis, int n_a, int n_b, int stride, double* xs, double* ys) {
    const int tid = (int)threadIdx.x, R = n_a + n_b;
    for (int j = tid; j < n_b; j += kMetaBlock) ys[j] = 0.0;
    for (int i = tid; i < n_a; i += kMetaBlock) { const double t = T[(size_t)n_a * stride + n_b + i]; xs[i] = t > 0.0 ? t : 0.0; }
    __syncthreads();
    for (int i = tid; i < n_a; i += kMetaBlock) {
        const int b = basis[i];
        if (b < n_b) { const double t = T[(size_t)i * stride + R]; ys[b] = t > 0.0 ? t : 0.0; }
    }
    __syncthreads();
}

// the outputs of game g.  status 1: the saddle point; otherwise xs / ys (LDS) hold meta_extract's values
__device__ __forceinline__ void meta_finish(const MetaIO& IO, int g, int status, int pivots, int istar, int jstar, double amax,
                                            double* xs, double* ys, MetaRed* red) {
    const int tid = (int)threadIdx.x, n_a = IO.n_a, n_b = IO.n_b;
    const double* A = IO.A + (size_t)g * n_a * n_b;
    double* x = IO.x + (size_t)g * n_a;
    double* y = IO.y + (size_t)g * n_b;
    if (status == 1) {
        for (int i = tid; i < n_a; i += kMetaBlock) x[i] = i == istar ? 1.0 : 0.0;
        for (int j = tid; j < n_b; j += kMetaBlock) y[j] = j == jstar ? 1.0 : 0.0;
        if (tid == 0) {
            const double v = A[(size_t)istar * n_b + jstar];
            IO.value[g] = v; IO.lo[g] = v; IO.hi[g] = v; IO.pivots[g] = 0; IO.status[g] = 1;
        }
        return;
    }
    if (tid == 0) {                                                     // the sums are sequential, in index order from 0.0
        double sx = 0.0, sy = 0.0;
        for (int i = 0; i < n_a; ++i) sx = sx + xs[i];
        for (int j = 0; j < n_b; ++j) sy = sy + ys[j];
        red->v[0] = sx; red->v[1] = sy;
    }
    __syncthreads();
    const double sx = red->v[0], sy = red->v[1];
    __syncthreads();
    for (int i = tid; i < n_a; i += kMetaBlock) { const double t = sx > 0.0 ? xs[i] / sx : 1.0 / (double)n_a; xs[i] = t; x[i] = t; }
    for (int j = tid; j < n_b; j += kMetaBlock) { const double t = sy > 0.0 ? ys[j] / sy : 1.0 / (double)n_b; ys[j] = t; y[j] = t; }
    __syncthreads();
    const double inf = __builtin_huge_val();
    double lo = inf; int k = INT_MAX;
    for (int j = tid; j < n_b; j += kMetaBlock) {                       // (x^T A)_j: consecutive lanes on consecutive columns
        double s = 0.0;
        for (int i = 0; i < n_a; ++i) s = s + xs[i] * A[(size_t)i * n_b + j];
        if (meta_before<false>(s, j, lo, k)) { lo = s; k = j; }
    }
    meta_block_arg<false>(lo, k, red);
    double hi = -inf; k = INT_MAX;
    for (int i = tid; i < n_a; i += kMetaBlock) {                       // (A y)_i
        const double* a = A + (size_t)i * n_b;
        double s = 0.0;
        for (int j = 0; j < n_b; ++j) s = s + a[j] * ys[j];
        if (meta_before<true>(s, i, hi, k)) { hi = s; k = i; }
    }
    meta_block_arg<true>(hi, k, red);
    if (tid == 0) {
        const double eps = 1e-10 * (amax > 1.0 ? amax : 1.0);
        IO.value[g] = 0.5 * (lo + hi); IO.lo[g] = lo; IO.hi[g] = hi; IO.pivots[g] = pivots;
        IO.status[g] = status == 3 ? 3 : (hi - lo <= eps ? 0 : 2);
    }
}

// ---- the LDS path: a workgroup per game, the tableau in dynamic LDS (meta_lds_bytes), one launch -------------------------
extern __shared__ double meta_smem[];
__global__ __launch_bounds__(kMetaBlock) void meta_lds_kernel(const MetaIO IO) {
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int n_a = IO.n_a, n_b = IO.n_b, stride = IO.stride, rows = IO.rows;
    MetaRed* red = reinterpret_cast<MetaRed*>(meta_smem);
    double* T = meta_smem + 16;
    double* prow = T + rows * stride;
    double* fcol = prow + stride;
    int32_t* basis = reinterpret_cast<int32_t*>(fcol + rows);
    int istar = 0, jstar = 0; double amax = 0.0;
    int status = 1, pivots = 0;
    if (!meta_setup(IO.A + (size_t)g * n_a * n_b, n_a, n_b, stride, T, basis, red, istar, jstar, amax)) {
        for (;;) {
            int c = 0, r = 0;
            const int res = meta_select(T, n_a, n_b, stride, pivots, IO.max_pivots, prow, fcol, red, c, r);
            if (res) { status = res == 3 ? 3 : -1; break; }
            int i = 0, j = tid;                                         // row-major, consecutive lanes on consecutive columns
            while (j >= stride) { j -= stride; ++i; }
            while (i < rows) {
                double* p = T + i * stride + j;
                *p = meta_entry(*p, fcol[i], prow[j], i == r, j == c);
                j += kMetaBlock;
                while (j >= stride) { j -= stride; ++i; }
            }
            if (tid == 0) basis[r] = c;
            ++pivots;
            __syncthreads();
        }
        meta_extract(T, basis, n_a, n_b, stride, prow, prow + n_a);     // the pivot row's place: stride >= n_a + n_b + 2
    }
    meta_finish(IO, g, status, pivots, istar, jstar, amax, prow, prow + n_a, red);
}

// ---- the global path --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMetaBlock) void meta_setup_kernel(const MetaIO IO) {
    __shared__ MetaRed red;
    const int g = (int)blockIdx.x;
    int istar = 0, jstar = 0; double amax = 0.0;
    const bool saddle = meta_setup(IO.A + (size_t)g * IO.n_a * IO.n_b, IO.n_a, IO.n_b, IO.stride, IO.T + (size_t)g * IO.rows * IO.stride,
                                   IO.basis + (size_t)g * IO.n_a, &red, istar, jstar, amax);
    if (threadIdx.x == 0) {
        int32_t* rec = IO.rec + (size_t)g * kMetaRec;
        rec[kMetaClosed] = saddle ? 1 : 0; rec[kMetaStatus] = saddle ? 1 : -1; rec[kMetaPivots] = 0;
        rec[kMetaCol] = 0; rec[kMetaRow] = 0; rec[kMetaIStar] = istar; rec[kMetaJStar] = jstar;
        IO.amax[g] = amax;
    }
}

// a workgroup per game: the pivot record, basis[r], the pivot count, and the side buffers the update reads — the update
// never reads what another workgroup is overwriting
__global__ __launch_bounds__(kMetaBlock) void meta_select_kernel(const MetaIO IO) {
    __shared__ MetaRed red;
    const int g = (int)blockIdx.x;
    int32_t* rec = IO.rec + (size_t)g * kMetaRec;
    if (rec[kMetaClosed]) return;
    const int pivots = rec[kMetaPivots];
    int c = 0, r = 0;
    const int res = meta_select(IO.T + (size_t)g * IO.rows * IO.stride, IO.n_a, IO.n_b, IO.stride, pivots, IO.max_pivots,
                                IO.prow + (size_t)g * IO.stride, IO.fcol + (size_t)g * IO.rows, &red, c, r);
    if (threadIdx.x == 0) {
        if (res) { rec[kMetaClosed] = 1; rec[kMetaStatus] = res == 3 ? 3 : -1; }
        else { rec[kMetaCol] = c; rec[kMetaRow] = r; rec[kMetaPivots] = pivots + 1; IO.basis[(size_t)g * IO.n_a + r] = c; }
    }
}

// grid (tiles of 16 rows x 256 columns, games): the rank-1 update, 8-byte accesses, consecutive lanes on consecutive columns
__global__ __launch_bounds__(kMetaBlock) void meta_update_kernel(const MetaIO IO) {
    const int g = (int)blockIdx.y;
    const int32_t* rec = IO.rec + (size_t)g * kMetaRec;
    if (rec[kMetaClosed]) return;
    const int c = rec[kMetaCol], r = rec[kMetaRow];
    const int col_tiles = (IO.stride + kMetaBlock - 1) / kMetaBlock;
    const int j = (int)(blockIdx.x % (unsigned)col_tiles) * kMetaBlock + (int)threadIdx.x;
    const int i0 = (int)(blockIdx.x / (unsigned)col_tiles) * kMetaTileRows;
    if (j >= IO.stride) return;
    const double p = IO.prow[(size_t)g * IO.stride + j];
    const double* f = IO.fcol + (size_t)g * IO.rows;
    double* T = IO.T + (size_t)g * IO.rows * IO.stride + j;
    const int i1 = i0 + kMetaTileRows < IO.rows ? i0 + kMetaTileRows : IO.rows;
    for (int i = i0; i < i1; ++i) {
        double* t = T + (size_t)i * IO.stride;
        *t = meta_entry(*t, f[i], p, i == r, j == c);
    }
}

// one workgroup: the games of the pass that still pivot, added to *open (the host cleared it)
__global__ __launch_bounds__(kMetaBlock) void meta_count_kernel(const MetaIO IO) {
    int n = 0;
    for (int g = (int)threadIdx.x; g < IO.games; g += kMetaBlock) n += IO.rec[(size_t)g * kMetaRec + kMetaClosed] ? 0 : 1;
    if (n) atomicAdd(IO.open, n);
}

// a workgroup per game, (n_a + n_b) * 8 bytes of dynamic LDS for the two strategies
__global__ __launch_bounds__(kMetaBlock) void meta_finish_kernel(const MetaIO IO) {
    __shared__ MetaRed red;
    const int g = (int)blockIdx.x;
    const int32_t* rec = IO.rec + (size_t)g * kMetaRec;
    const int status = rec[kMetaStatus];
    double* xs = meta_smem;
    double* ys = meta_smem + IO.n_a;
    if (status != 1)
        meta_extract(IO.T + (size_t)g * IO.rows * IO.stride, IO.basis + (size_t)g * IO.n_a, IO.n_a, IO.n_b, IO.stride, xs, ys);
    meta_finish(IO, g, status, rec[kMetaPivots], rec[kMetaIStar], rec[kMetaJStar], IO.amax[g], xs, ys, &red);
}

}  // namespace soccer
