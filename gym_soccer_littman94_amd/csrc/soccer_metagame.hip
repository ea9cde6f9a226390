// soccer_metagame.hip — soccer_solve_meta_games: the maximin mixtures of n_a x n_b zero-sum matrix games (see soccer_handle.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "soccer_handle.hpp"
#include "soccer_metagame_kernels.hpp"

namespace {

constexpr int kMetaPivotsPerSync = 64;          // the library's choice of pivots_per_sync
constexpr size_t kMetaPassBytes = (size_t)1 << 30;

// what a pass of `games` games needs, in elements, in the order of soccer_handle::mg_need
void meta_need(int games, int n_a, int n_b, bool lds, size_t need[5]) {
    const size_t g = (size_t)games, rows = (size_t)n_a + 1, stride = (size_t)meta_stride(n_a, n_b);
    need[0] = g * (size_t)n_a * (size_t)n_b;                            // A
    need[1] = lds ? 0 : g * rows * stride;                              // T
    need[2] = g * (size_t)std::max(n_a + 1, n_b);                       // per game and row or column: x, y, basis, fcol
    need[3] = g * stride;                                               // prow
    need[4] = g;                                                        // per game: the records and the scalars
}

int meta_buffers(soccer_handle* h, const size_t need[5]) {
    bool enough = true;
    for (int i = 0; i < 5; ++i) enough = enough && need[i] <= h->mg_need[i];
    if (enough) return SOCCER_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    size_t want[5];
    for (int i = 0; i < 5; ++i) want[i] = std::max(need[i], h->mg_need[i]);
    h->mg_bufs.clear();
    for (int i = 0; i < 5; ++i) h->mg_need[i] = 0;
    const size_t games = want[4];
    int rc = h->mg_bufs.alloc(h, want[0], &h->mg_A);
    if (!rc) rc = h->mg_bufs.alloc(h, want[1], &h->mg_T);
    if (!rc) rc = h->mg_bufs.alloc(h, want[2], &h->mg_x);
    if (!rc) rc = h->mg_bufs.alloc(h, want[2], &h->mg_y);
    if (!rc) rc = h->mg_bufs.alloc(h, want[2], &h->mg_fcol);
    if (!rc) rc = h->mg_bufs.alloc(h, want[2], &h->mg_basis);
    if (!rc) rc = h->mg_bufs.alloc(h, want[3], &h->mg_prow);
    if (!rc) rc = h->mg_bufs.alloc(h, games * 4, &h->mg_scal);
    if (!rc) rc = h->mg_bufs.alloc(h, games * (kMetaRec + 2) + 1, &h->mg_int);
    if (rc) { h->mg_bufs.clear(); return rc; }
    for (int i = 0; i < 5; ++i) h->mg_need[i] = want[i];
    return SOCCER_OK;
}

}  // namespace

extern "C" int soccer_solve_meta_games(soccer_handle* h, int64_t n_games, int32_t n_a, int32_t n_b, const double* A, int32_t max_pivots,
                                       int32_t path, int32_t pivots_per_sync, const soccer_meta_game_result* out) {
    const char* what = "soccer_solve_meta_games";
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "%s during graph capture", what);
    if (n_a < 1 || n_a > SOCCER_META_MAX_POLICIES || n_b < 1 || n_b > SOCCER_META_MAX_POLICIES)
        return fail(h, SOCCER_E_INVALID, "%s: n_a and n_b must be 1 .. %d, not %d and %d", what, SOCCER_META_MAX_POLICIES, n_a, n_b);
    if (n_games < 0) return fail(h, SOCCER_E_INVALID, "n_games must be >= 0");
    if (max_pivots < 1) return fail(h, SOCCER_E_INVALID, "max_pivots must be >= 1");
    if (path < 0 || path > 2) return fail(h, SOCCER_E_INVALID, "%s: path must be 0 (the library chooses), 1 (LDS) or 2 (global), not %d", what, path);
    if (pivots_per_sync < 0) return fail(h, SOCCER_E_INVALID, "%s: pivots_per_sync must be >= 0 (0: the library chooses), not %d", what, pivots_per_sync);
    if (n_games == 0) return SOCCER_OK;
    if (!A) return fail(h, SOCCER_E_INVALID, "A is NULL");
    const size_t cells = (size_t)n_a * n_b;
    for (int64_t g = 0; g < n_games; ++g) {
        const double* a = A + (size_t)g * cells;
        double lo_a = a[0], hi_a = a[0];
        for (size_t k = 0; k < cells; ++k) {
            if (!std::isfinite(a[k]))
                return fail(h, SOCCER_E_INVALID, "%s: A[game %lld][row %d][column %d] is not finite", what, (long long)g, (int)(k / n_b), (int)(k % n_b));
            lo_a = a[k] < lo_a ? a[k] : lo_a;
            hi_a = a[k] > hi_a ? a[k] : hi_a;
        }
        if (!std::isfinite(hi_a - lo_a))                                // the tableau would divide by it
            return fail(h, SOCCER_E_INVALID, "%s: A[game %lld]: max A - min A is not finite (%g - %g)", what, (long long)g, hi_a, lo_a);
    }
    const size_t lds = meta_lds_bytes(n_a, n_b);
    const bool fits = lds <= h->lds_limit;
    if (path == 1 && !fits)
        return fail(h, SOCCER_E_INVALID, "%s: a %d x %d game does not fit the LDS kernel (%zu bytes, the limit is %zu)", what, n_a, n_b, lds, h->lds_limit);
    const bool use_lds = path == 1 || (path == 0 && fits);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const int rows = n_a + 1, stride = meta_stride(n_a, n_b);
    // a pass: the matrices and (the global path) the tableaux stay at or under 1 GiB each; grid.y bounds the global path
    const size_t per_game = 8 * std::max(cells, use_lds ? (size_t)0 : (size_t)rows * stride);
    const int64_t cap = use_lds ? ((int64_t)1 << 20) : 32768;
    const int per_pass = (int)std::min<int64_t>(std::min<int64_t>(n_games, cap), std::max<int64_t>(1, (int64_t)(kMetaPassBytes / per_game)));
    size_t need[5];
    meta_need(per_pass, n_a, n_b, use_lds, need);
    if (int rc = meta_buffers(h, need)) return rc;
    if (use_lds && lds > 48 * 1024)
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&meta_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int per_sync = pivots_per_sync ? pivots_per_sync : kMetaPivotsPerSync;
    static const soccer_meta_game_result none{};
    const soccer_meta_game_result& o = out ? *out : none;
    MetaIO io{};
    io.A = h->mg_A; io.T = h->mg_T; io.prow = h->mg_prow; io.fcol = h->mg_fcol; io.basis = h->mg_basis; io.x = h->mg_x; io.y = h->mg_y;
    io.rec = h->mg_int; io.pivots = h->mg_int + (size_t)per_pass * kMetaRec; io.status = io.pivots + per_pass; io.open = io.status + per_pass;
    io.value = h->mg_scal; io.lo = io.value + per_pass; io.hi = io.lo + per_pass; io.amax = io.hi + per_pass;
    io.n_a = n_a; io.n_b = n_b; io.rows = rows; io.cols = n_a + n_b + 2; io.stride = stride; io.max_pivots = max_pivots;
    std::vector<int32_t> status_host((size_t)per_pass);
    int64_t stopped = 0;
    for (int64_t first = 0; first < n_games; first += per_pass) {
        const int games = (int)std::min<int64_t>(per_pass, n_games - first);
        io.games = games;
        HIP_TRY(h, hipMemcpyAsync(h->mg_A, A + (size_t)first * cells, (size_t)games * cells * 8, hipMemcpyHostToDevice, h->stream));
        if (use_lds) {
            hipLaunchKernelGGL(meta_lds_kernel, dim3((unsigned)games), dim3(kMetaBlock), lds, h->stream, io);
        } else {
            hipLaunchKernelGGL(meta_setup_kernel, dim3((unsigned)games), dim3(kMetaBlock), 0, h->stream, io);
            const unsigned tiles = (unsigned)((stride + kMetaBlock - 1) / kMetaBlock) * (unsigned)((rows + kMetaTileRows - 1) / kMetaTileRows);
            // every game stops within max_pivots + 1 selects; a batch of pivots is enqueued blind, then one int32 is read
            int32_t open = games;
            for (int64_t done = 0; open && done <= (int64_t)max_pivots; done += per_sync) {
                const int nb = (int)std::min<int64_t>(per_sync, (int64_t)max_pivots + 1 - done);
                for (int k = 0; k < nb; ++k) {
                    hipLaunchKernelGGL(meta_select_kernel, dim3((unsigned)games), dim3(kMetaBlock), 0, h->stream, io);
                    hipLaunchKernelGGL(meta_update_kernel, dim3(tiles, (unsigned)games), dim3(kMetaBlock), 0, h->stream, io);
                }
                HIP_TRY(h, hipMemsetAsync(io.open, 0, sizeof(int32_t), h->stream));
                hipLaunchKernelGGL(meta_count_kernel, dim3(1), dim3(kMetaBlock), 0, h->stream, io);
                HIP_TRY(h, hipGetLastError());
                HIP_TRY(h, hipMemcpyAsync(&open, io.open, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
                HIP_TRY(h, hipStreamSynchronize(h->stream));
            }
            if (open) return fail(h, SOCCER_E_HIP, "%s: %d games still pivot after max_pivots + 1 selections", what, (int)open);
            hipLaunchKernelGGL(meta_finish_kernel, dim3((unsigned)games), dim3(kMetaBlock), (size_t)(n_a + n_b) * 8, h->stream, io);
        }
        HIP_TRY(h, hipGetLastError());
        const size_t g0 = (size_t)first, n = (size_t)games;
        if (o.value) HIP_TRY(h, hipMemcpyAsync(o.value + g0, io.value, n * 8, hipMemcpyDeviceToHost, h->stream));
        if (o.lo) HIP_TRY(h, hipMemcpyAsync(o.lo + g0, io.lo, n * 8, hipMemcpyDeviceToHost, h->stream));
        if (o.hi) HIP_TRY(h, hipMemcpyAsync(o.hi + g0, io.hi, n * 8, hipMemcpyDeviceToHost, h->stream));
        if (o.x) HIP_TRY(h, hipMemcpyAsync(o.x + g0 * n_a, io.x, n * n_a * 8, hipMemcpyDeviceToHost, h->stream));
        if (o.y) HIP_TRY(h, hipMemcpyAsync(o.y + g0 * n_b, io.y, n * n_b * 8, hipMemcpyDeviceToHost, h->stream));
        if (o.pivots) HIP_TRY(h, hipMemcpyAsync(o.pivots + g0, io.pivots, n * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemcpyAsync(status_host.data(), io.status, n * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (size_t g = 0; g < n; ++g) {
            if (o.status) o.status[g0 + g] = status_host[g];
            stopped += status_host[g] == 3;
        }
    }
    if (stopped) return fail(h, SOCCER_E_STATE, "%s: %lld of %lld games stopped at max_pivots = %d", what, (long long)stopped,
                             (long long)n_games, max_pivots);
    return SOCCER_OK;
}
