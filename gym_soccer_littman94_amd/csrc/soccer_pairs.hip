// soccer_pairs.hip — the pair evaluators, which solve every pair (pi_a[i], pi_b[j]) of two sets of mixed policies, on one host skeleton: cross-play, match outcomes, state occupancy and policy gradients, and gradient play on the last (see soccer_handle.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstring>
#include <vector>

#include "soccer_handle.hpp"
#include "soccer_pair_kernels.hpp"

// ------------------------------------------------------------------------------------------------
// What the evaluators share (two-player handles).  Each pair is soccer_evaluate_policies' kind of iteration, solved to the
// bits it has alone; the work is laid out the other way round (a lane owns a pair), the policies are uploaded once, a matrix
// larger than a pass is solved pass after pass over the same buffers, and the stopping sweeps are found on the device: a
// batch of sweeps costs the host one 4-byte read.

// every check but those of the policies; `discount` names the argument that gamma is
static int pair_check(soccer_handle* h, const char* what, const char* discount, double gamma, int32_t n_a, int32_t n_b, double theta,
                      int32_t max_sweeps, int32_t pairs_per_pass) {
    if (int rc = minimax_check(h, what, 0.0)) return rc;
    if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(h, SOCCER_E_INVALID, "%s must be in [0, 1]", discount);
    if (n_a < 1 || n_a > SOCCER_CROSS_MAX_POLICIES || n_b < 1 || n_b > SOCCER_CROSS_MAX_POLICIES)
        return fail(h, SOCCER_E_INVALID, "%s: the number of policies of each player must be 1 .. %d, not %d and %d", what,
                    SOCCER_CROSS_MAX_POLICIES, n_a, n_b);
    if (max_sweeps < 1) return fail(h, SOCCER_E_INVALID, "max_sweeps must be >= 1");
    if (!(theta >= 0.0)) return fail(h, SOCCER_E_INVALID, "theta must be >= 0");
    if (pairs_per_pass < 0 || pairs_per_pass % 64)
        return fail(h, SOCCER_E_INVALID, "%s: pairs_per_pass must be 0 (the library chooses) or a positive multiple of 64, not %d", what, pairs_per_pass);
    return SOCCER_OK;
}

// the pairs of a pass: the caller's, or the library's choice, under which the buffers that a pass sweeps over and fills,
// `bytes` for every pair and state, stay at or under 1 GiB; never more than the matrix in whole waves
static int pass_pairs(int32_t pairs_per_pass, size_t bytes, int nS, int total) {
    const int per_pass = pairs_per_pass ? pairs_per_pass : std::max(64, (int)(((size_t)1 << 30) / (bytes * nS) / 64 * 64));
    return std::min(per_pass, (total + 63) / 64 * 64);
}

// what an evaluator's family is made of besides the core: the rows a pair has in an iterate and in the values buffer, and
// whether the policies are kept transposed too
struct PairShape { size_t rows, width; bool transposed; };

// Grows a family to `policies`, a pass of `stride` pairs and, with `values`, the values buffer: nothing is given up that is
// held already, and what is held stays when it suffices.  own(policies, stride) allocates from F.bufs what only this
// evaluator has.  No result depends on a stride an earlier, larger pass left.
template <class Own>
static int pair_buffers(soccer_handle* h, PairBufs& F, const PairShape& shape, int policies, int stride, bool values, Own own) {
    if (policies <= F.policies && stride <= F.pass.stride && (!values || F.has_values)) return SOCCER_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    policies = std::max(policies, F.policies); stride = std::max(stride, F.pass.stride); values = values || F.has_values;
    F.bufs.clear();
    F.policies = 0; F.pass.stride = 0; F.has_values = false;
    const size_t n = (size_t)stride, block = (size_t)policies * h->mm.nS * 5;
    int rc = F.bufs.alloc(h, block, &F.pol);
    if (!rc && shape.transposed) rc = F.bufs.alloc(h, block, &F.polT);
    for (int i = 0; i < 2 && !rc; ++i) rc = F.bufs.alloc(h, shape.rows * n, &F.pass.buf[i]);
    if (!rc) rc = F.bufs.alloc(h, n * (kMinimaxBatch + 1), &F.pass.words);
    if (!rc) rc = F.bufs.alloc(h, n, &F.pass.done);
    if (!rc) rc = F.bufs.alloc(h, (size_t)1, &F.pass.open);
    if (!rc) rc = F.bufs.alloc(h, n, &F.iter);
    if (!rc) rc = own((size_t)policies, n);
    if (!rc && values) rc = F.bufs.alloc(h, shape.width * n, &F.values);
    if (rc) { F.bufs.clear(); return rc; }
    F.policies = policies; F.pass.stride = stride; F.has_values = values;
    return SOCCER_OK;
}

// a call's policies ([n][nS][5] where `kind` says) into the family, row 0 of each as zeros, and where the family keeps them
// transposed as well, [n][nS][5] -> [nS][5][n] on the device
static int pair_policies(soccer_handle* h, const PairBufs& F, int n_a, const double* pa, int n_b, const double* pb,
                         hipMemcpyKind kind = hipMemcpyHostToDevice) {
    const size_t rows = (size_t)h->mm.nS * 5;
    if (int rc = response_upload(h, F.pol, pa, n_a, kind)) return rc;
    if (int rc = response_upload(h, F.pol + (size_t)n_a * rows, pb, n_b, kind)) return rc;
    if (!F.polT) return SOCCER_OK;
    for (int side = 0; side < 2; ++side) {
        OccupancyPolicyIO pio{};
        pio.pol = F.pol + (side ? (size_t)n_a * rows : 0); pio.polT = F.polT + (side ? (size_t)n_a * rows : 0);
        pio.n = side ? n_b : n_a; pio.rows = (int32_t)rows;
        const size_t cells = rows * (size_t)pio.n;
        hipLaunchKernelGGL(occupancy_transpose_kernel, dim3((unsigned)((cells + kCrossBlock - 1) / kCrossBlock)), dim3(kCrossBlock), 0, h->stream, pio);
    }
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

// the initial states' observation indices into an argument block
template <class IO>
static void fill_isd(const soccer_handle* h, IO& io) {
    io.n_isd = h->rules.n_isd;
    for (int i = 0; i < h->rules.n_isd; ++i) io.isd[i] = (int32_t)h->rules.isd_obs[i];
}

// everything of a sweep over the family's policies but the pass and the buffers of the sweep: cross_sweep_kernel's and
// match_sweep_kernel's, and occupancy_sweep_kernel's
static CrossIO cross_io(const soccer_handle* h, const PairBufs& F, int n_a, int n_b, double gamma, double theta) {
    CrossIO io{};
    io.offset = h->mm.offset; io.list = h->mm.list; io.x = F.pol; io.y = F.pol + (size_t)n_a * h->mm.nS * 5; io.gamma = gamma; io.theta = theta;
    io.nS = h->mm.nS; io.n_b = n_b; io.stride = F.pass.stride; io.last = n_a * n_b - 1;
    return io;
}

static OccupancyIO occupancy_io(const soccer_handle* h, const PairBufs& F, int n_a, int n_b, double c, double theta) {
    OccupancyIO io{};
    io.in_offset = h->in_offset; io.in_list = h->in_list; io.xT = F.polT; io.yT = F.polT + (size_t)n_a * h->mm.nS * 5; io.c = c; io.theta = theta;
    fill_isd(h, io);
    io.mu = 1.0 / (double)h->rules.n_isd;
    io.nS = h->mm.nS; io.n_a = n_a; io.n_b = n_b; io.stride = F.pass.stride; io.last = n_a * n_b - 1;
    return io;
}

static inline unsigned pair_blocks(int pairs) { return (unsigned)((pairs + kCrossBlock - 1) / kCrossBlock); }

// One pass of a solve whose pairs stop one by one: both buffers cleared, then batches of sweeps until every pair has stopped
// or max_sweeps is reached, the stopping sweeps found on the device (cross_batch_kernel) and read back as one count per
// batch.  An iterate has `rows` rows; sweep(k, in, out, delta, prev) launches sweep k; open_left (may be NULL) takes the
// number of pairs still open at the end.
template <class Sweep>
static int solve_pass(soccer_handle* h, const PassBufs& B, size_t rows, int pairs, double theta, int32_t max_sweeps, Sweep sweep, int32_t* open_left) {
    const size_t stride = (size_t)B.stride;
    CrossBatchIO bio{};
    bio.words = B.words; bio.done_at = B.done; bio.open = B.open; bio.theta = theta; bio.stride = B.stride; bio.n_words = kMinimaxBatch + 1;
    bio.pairs = pairs;
    HIP_TRY(h, hipMemsetAsync(B.buf[0], 0, rows * stride * 8, h->stream));                 // the iterate before sweep 1 is 0
    HIP_TRY(h, hipMemsetAsync(B.buf[1], 0, rows * stride * 8, h->stream));
    HIP_TRY(h, hipMemsetAsync(B.open, 0, sizeof(int32_t), h->stream));
    bio.k0 = 0; bio.nb = 0;
    hipLaunchKernelGGL(cross_batch_kernel, dim3(pair_blocks(pairs)), dim3(kCrossBlock), 0, h->stream, bio);
    int32_t k0 = 1, open = pairs;                                                          // k0: first sweep of the batch
    while (k0 <= max_sweeps && open) {
        const int nb = (int)std::min<int64_t>(kMinimaxBatch, (int64_t)max_sweeps - k0 + 1);
        for (int j = 1; j <= nb; ++j) {
            const int32_t k = k0 + j - 1;
            sweep(k, B.buf[(k - 1) & 1], B.buf[k & 1], B.words + (size_t)j * stride, B.words + (size_t)(j - 1) * stride);
        }
        HIP_TRY(h, hipMemsetAsync(B.open, 0, sizeof(int32_t), h->stream));
        bio.k0 = k0; bio.nb = nb;
        hipLaunchKernelGGL(cross_batch_kernel, dim3(pair_blocks(pairs)), dim3(kCrossBlock), 0, h->stream, bio);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(&open, B.open, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        k0 += nb;
    }
    if (open_left) *open_left = open;
    return SOCCER_OK;
}

// cross-play's pass over device-resident policies: io holds everything but the buffers of a sweep
static int cross_solve_pass(soccer_handle* h, CrossIO io, const PassBufs& B, int32_t max_sweeps, int32_t* open_left) {
    const dim3 grid((unsigned)((io.nS + kCrossWaves - 1) / kCrossWaves), (unsigned)((io.pairs + 63) / 64));
    return solve_pass(h, B, (size_t)io.nS, io.pairs, io.theta, max_sweeps,
                      [&](int32_t, const double* in, double* out, unsigned long long* delta, const unsigned long long* prev) {
                          io.V = in; io.V_out = out; io.delta = delta; io.prev = prev;
                          hipLaunchKernelGGL(cross_sweep_kernel, grid, dim3(kCrossBlock), 0, h->stream, io);
                      }, open_left);
}

// the match outcomes', likewise: three channels to a state, and a pair's word the maximum over them, so cross_batch_kernel serves it unchanged
static int match_solve_pass(soccer_handle* h, CrossIO io, const PassBufs& B, int32_t max_sweeps, int32_t* open_left) {
    const dim3 grid((unsigned)((io.nS + kCrossWaves - 1) / kCrossWaves), (unsigned)((io.pairs + 63) / 64));
    return solve_pass(h, B, (size_t)kMatchChannels * io.nS, io.pairs, io.theta, max_sweeps,
                      [&](int32_t, const double* in, double* out, unsigned long long* delta, const unsigned long long* prev) {
                          io.V = in; io.V_out = out; io.delta = delta; io.prev = prev;
                          hipLaunchKernelGGL(match_sweep_kernel, grid, dim3(kCrossBlock), 0, h->stream, io);
                      }, open_left);
}

// the occupancy's, likewise (over the transposed policies)
static int occupancy_solve_pass(soccer_handle* h, OccupancyIO io, const PassBufs& B, int32_t max_sweeps, int32_t* open_left) {
    const dim3 grid((unsigned)((io.nS + kCrossWaves - 1) / kCrossWaves), (unsigned)((io.pairs + 63) / 64));
    return solve_pass(h, B, (size_t)io.nS, io.pairs, io.theta, max_sweeps,
                      [&](int32_t, const double* in, double* out, unsigned long long* delta, const unsigned long long* prev) {
                          io.D = in; io.D_out = out; io.delta = delta; io.prev = prev;
                          hipLaunchKernelGGL(occupancy_sweep_kernel, grid, dim3(kCrossBlock), 0, h->stream, io);
                      }, open_left);
}

// The split of a matrix of `total` pairs into passes of per_pass: pass(first, pairs, &open) solves the `pairs` pairs from
// matrix index `first` on, hands their results to the caller and says how many it left open; after(), behind the last pass,
// is the call's own ending; then the call is refused if any pair of any pass was left open.
template <class Pass, class After>
static int pair_passes(soccer_handle* h, const char* what, int total, int per_pass, int32_t max_sweeps, Pass pass, After after) {
    int64_t open_total = 0;
    for (int first = 0; first < total; first += per_pass) {
        int32_t open = 0;
        if (int rc = pass(first, std::min(per_pass, total - first), &open)) return rc;
        open_total += open;
    }
    if (int rc = after()) return rc;
    if (open_total) return fail(h, SOCCER_E_STATE, "%s: %lld of %d pairs had not converged after max_sweeps = %d sweeps", what,
                                (long long)open_total, total, max_sweeps);
    return SOCCER_OK;
}

template <class Pass>
static int pair_passes(soccer_handle* h, const char* what, int total, int per_pass, int32_t max_sweeps, Pass pass) {
    return pair_passes(h, what, total, per_pass, max_sweeps, pass, [] { return (int)SOCCER_OK; });
}

// ------------------------------------------------------------------------------------------------
// cross-play: player A's value of every pair, soccer_evaluate_policies' iteration with a sweep of cross_sweep_kernel.
extern "C" int soccer_cross_play(soccer_handle* h, int32_t n_a, const double* pi_a, int32_t n_b, const double* pi_b, double theta,
                                 double discount_factor, int32_t max_sweeps, int32_t pairs_per_pass, double* payoff, double* V,
                                 int32_t* iterations) {
    const char* what = "soccer_cross_play";
    if (int rc = pair_check(h, what, "discount_factor", discount_factor, n_a, n_b, theta, max_sweeps, pairs_per_pass)) return rc;
    if (int rc = response_rows(h, what, "pi_a", n_a, pi_a)) return rc;
    if (int rc = response_rows(h, what, "pi_b", n_b, pi_b)) return rc;
    if (int rc = minimax_prepare(h)) return rc;
    const int nS = h->mm.nS, total = n_a * n_b;
    const int per_pass = pass_pairs(pairs_per_pass, 16, nS, total);     // the two V buffers of a pass
    PairBufs& F = h->cross;
    CrossOwn& own = h->cross_own;
    if (int rc = pair_buffers(h, F, {(size_t)nS, (size_t)nS, false}, n_a + n_b, per_pass, V != nullptr,
                              [&](size_t, size_t stride) { return F.bufs.alloc(h, stride, &own.payoff); })) return rc;
    if (int rc = pair_policies(h, F, n_a, pi_a, n_b, pi_b)) return rc;
    CrossIO io = cross_io(h, F, n_a, n_b, discount_factor, theta);
    CrossFinishIO fio{};
    fio.V[0] = F.pass.buf[0]; fio.V[1] = F.pass.buf[1]; fio.done_at = F.pass.done; fio.payoff = own.payoff; fio.iterations = F.iter;
    fio.values = F.values; fio.nS = nS; fio.stride = F.pass.stride; fio.max_sweeps = max_sweeps;
    fill_isd(h, fio);
    return pair_passes(h, what, total, per_pass, max_sweeps, [&](int first, int pairs, int32_t* open) -> int {
        io.first = first; io.pairs = pairs; fio.pairs = pairs;
        if (int rc = cross_solve_pass(h, io, F.pass, max_sweeps, open)) return rc;         // V_0 = 0
        hipLaunchKernelGGL(cross_finish_kernel, dim3(pair_blocks(pairs)), dim3(kCrossBlock), 0, h->stream, fio);
        if (V) hipLaunchKernelGGL(cross_values_kernel, dim3((unsigned)((pairs + 63) / 64), (unsigned)((nS + 63) / 64)), dim3(kCrossBlock), 0, h->stream, fio);
        HIP_TRY(h, hipGetLastError());
        if (payoff) HIP_TRY(h, hipMemcpyAsync(payoff + first, own.payoff, (size_t)pairs * 8, hipMemcpyDeviceToHost, h->stream));
        if (iterations) HIP_TRY(h, hipMemcpyAsync(iterations + first, F.iter, (size_t)pairs * 4, hipMemcpyDeviceToHost, h->stream));
        if (V) HIP_TRY(h, hipMemcpyAsync(V + (size_t)first * nS, F.values, (size_t)pairs * nS * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return SOCCER_OK;
    });
}

// ------------------------------------------------------------------------------------------------
// match outcomes: for every pair the probability that A, and that B, scores the goal that ends the game, and the expected
// number of steps it lasts, when every step is followed by another with probability continue_prob.  Three channels W_A, W_B
// and L to a state in the iterate; a sweep is one launch of match_sweep_kernel, which reads every list entry once for the
// three sums.
extern "C" int soccer_match_outcomes(soccer_handle* h, int32_t n_a, const double* pi_a, int32_t n_b, const double* pi_b, double theta,
                                     double continue_prob, int32_t max_sweeps, int32_t pairs_per_pass, double* win_a, double* win_b,
                                     double* length, double* values, int32_t* iterations) {
    const char* what = "soccer_match_outcomes";
    if (int rc = pair_check(h, what, "continue_prob", continue_prob, n_a, n_b, theta, max_sweeps, pairs_per_pass)) return rc;
    if (int rc = response_rows(h, what, "pi_a", n_a, pi_a)) return rc;
    if (int rc = response_rows(h, what, "pi_b", n_b, pi_b)) return rc;
    if (int rc = minimax_prepare(h)) return rc;
    const int nS = h->mm.nS, total = n_a * n_b;
    const int per_pass = pass_pairs(pairs_per_pass, 16 * kMatchChannels, nS, total);   // the two three-channel buffers of a pass
    PairBufs& F = h->match;
    MatchOwn& own = h->match_own;
    const size_t rows = (size_t)kMatchChannels * nS;
    if (int rc = pair_buffers(h, F, {rows, rows, false}, n_a + n_b, per_pass, values != nullptr,
                              [&](size_t, size_t stride) { return F.bufs.alloc(h, kMatchChannels * stride, &own.kickoff); })) return rc;
    const int stride = F.pass.stride;
    if (int rc = pair_policies(h, F, n_a, pi_a, n_b, pi_b)) return rc;
    CrossIO io = cross_io(h, F, n_a, n_b, continue_prob, theta);
    MatchFinishIO fio{};
    fio.V[0] = F.pass.buf[0]; fio.V[1] = F.pass.buf[1]; fio.done_at = F.pass.done; fio.kickoff = own.kickoff; fio.iterations = F.iter;
    fio.values = F.values; fio.nS = nS; fio.stride = stride; fio.max_sweeps = max_sweeps;
    fill_isd(h, fio);
    double* const outs[kMatchChannels] = {win_a, win_b, length};
    return pair_passes(h, what, total, per_pass, max_sweeps, [&](int first, int pairs, int32_t* open) -> int {
        io.first = first; io.pairs = pairs; fio.pairs = pairs;
        if (int rc = match_solve_pass(h, io, F.pass, max_sweeps, open)) return rc;         // W_A = W_B = L = 0
        hipLaunchKernelGGL(match_finish_kernel, dim3(pair_blocks(pairs)), dim3(kCrossBlock), 0, h->stream, fio);
        if (values) hipLaunchKernelGGL(match_values_kernel, dim3((unsigned)((pairs + 63) / 64), (unsigned)((nS + 63) / 64), kMatchChannels),
                                       dim3(kCrossBlock), 0, h->stream, fio);
        HIP_TRY(h, hipGetLastError());
        for (int c = 0; c < kMatchChannels; ++c)
            if (outs[c]) HIP_TRY(h, hipMemcpyAsync(outs[c] + first, own.kickoff + (size_t)c * stride, (size_t)pairs * 8, hipMemcpyDeviceToHost, h->stream));
        if (iterations) HIP_TRY(h, hipMemcpyAsync(iterations + first, F.iter, (size_t)pairs * 4, hipMemcpyDeviceToHost, h->stream));
        if (values) HIP_TRY(h, hipMemcpyAsync(values + (size_t)first * rows, F.values, (size_t)pairs * rows * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return SOCCER_OK;
    });
}

// ------------------------------------------------------------------------------------------------
// state occupancy: for every pair the expected discounted number of visits to every state from kick-off, the dual of
// cross-play's value.  The sweep sums over in-lists, the two-player lists the other way round, which are built on the host
// once per handle (soccer_inlists.hpp) from a copy of the device's lists, and reads the policies transposed, so that the
// per-entry policy reads of occupancy_sweep_kernel are contiguous across the lanes.
static int build_occupancy_lists(soccer_handle* h) {
    if (h->in_lists.ready) return SOCCER_OK;
    const int nS = h->mm.nS;
    const size_t nkeys = (size_t)nS * 25;
    std::vector<int32_t> off(nkeys + 1);
    HIP_TRY(h, hipMemcpyAsync(off.data(), h->mm.offset, off.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::vector<PlanEntry> list((size_t)off[nkeys]);
    HIP_TRY(h, hipMemcpyAsync(list.data(), h->mm.list, list.size() * sizeof(PlanEntry), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::vector<int32_t> in_off; std::vector<InEntry> in_list;
    if (!build_inlists(nS, off.data(), list.data(), in_off, in_list))
        return fail(h, SOCCER_E_INVALID, "internal error: the two-player lists have an entry whose next state is not a state");
    h->in_lists.clear();
    int rc = h->in_lists.upload(h, in_off, &h->in_offset);
    if (!rc) rc = h->in_lists.upload(h, in_list, &h->in_list);
    if (rc) { h->in_lists.clear(); return rc; }
    h->in_lists.ready = true;
    return SOCCER_OK;
}

extern "C" int soccer_occupancy(soccer_handle* h, int32_t n_a, const double* pi_a, int32_t n_b, const double* pi_b, double theta,
                                double continue_prob, int32_t max_sweeps, int32_t pairs_per_pass, int32_t n_f, const double* features,
                                double* length, double* expect, double* occupancy, int32_t* iterations) {
    const char* what = "soccer_occupancy";
    if (int rc = pair_check(h, what, "continue_prob", continue_prob, n_a, n_b, theta, max_sweeps, pairs_per_pass)) return rc;
    if (n_f < 0 || n_f > SOCCER_OCC_MAX_FEATURES)
        return fail(h, SOCCER_E_INVALID, "%s: the number of features must be 0 .. %d, not %d", what, SOCCER_OCC_MAX_FEATURES, n_f);
    if (n_f > 0 && !features) return fail(h, SOCCER_E_INVALID, "%s: features is NULL", what);
    if (int rc = response_rows(h, what, "pi_a", n_a, pi_a)) return rc;
    if (int rc = response_rows(h, what, "pi_b", n_b, pi_b)) return rc;
    if (int rc = minimax_prepare(h)) return rc;
    if (int rc = build_occupancy_lists(h)) return rc;
    const int nS = h->mm.nS, total = n_a * n_b;
    const int sums = expect ? n_f : 0;                                  // the expectations that are formed
    const int per_pass = pass_pairs(pairs_per_pass, 16, nS, total);     // the two D buffers of a pass
    PairBufs& F = h->occupancy;
    OccupancyOwn& own = h->occupancy_own;
    if (int rc = pair_buffers(h, F, {(size_t)nS, (size_t)nS, true}, n_a + n_b, per_pass, occupancy != nullptr, [&](size_t, size_t stride) {
            int rc = F.bufs.alloc(h, stride, &own.length);
            if (!rc) rc = F.bufs.alloc(h, stride * SOCCER_OCC_MAX_FEATURES, &own.expect);
            if (!rc) rc = F.bufs.alloc(h, (size_t)SOCCER_OCC_MAX_FEATURES * nS, &own.features);
            return rc;
        })) return rc;
    const int stride = F.pass.stride;
    if (int rc = pair_policies(h, F, n_a, pi_a, n_b, pi_b)) return rc;
    if (sums) HIP_TRY(h, hipMemcpyAsync(own.features, features, (size_t)sums * nS * 8, hipMemcpyHostToDevice, h->stream));
    OccupancyIO io = occupancy_io(h, F, n_a, n_b, continue_prob, theta);
    OccupancyFinishIO fio{};
    fio.D[0] = F.pass.buf[0]; fio.D[1] = F.pass.buf[1]; fio.done_at = F.pass.done; fio.features = own.features;
    fio.length = length ? own.length : nullptr; fio.expect = own.expect; fio.iterations = F.iter;
    fio.nS = nS; fio.stride = stride; fio.max_sweeps = max_sweeps; fio.n_f = sums;
    CrossFinishIO vio{};                                                // cross_values_kernel's: D is laid out like cross-play's V
    vio.V[0] = F.pass.buf[0]; vio.V[1] = F.pass.buf[1]; vio.done_at = F.pass.done; vio.values = F.values;
    vio.nS = nS; vio.stride = stride; vio.max_sweeps = max_sweeps;
    return pair_passes(h, what, total, per_pass, max_sweeps, [&](int first, int pairs, int32_t* open) -> int {
        io.first = first; io.pairs = pairs; fio.pairs = pairs; vio.pairs = pairs;
        if (int rc = occupancy_solve_pass(h, io, F.pass, max_sweeps, open)) return rc;     // D_0 = 0, and row 0 of both for good
        hipLaunchKernelGGL(occupancy_finish_kernel, dim3(pair_blocks(pairs), (unsigned)(1 + sums)), dim3(kCrossBlock), 0, h->stream, fio);
        if (occupancy) hipLaunchKernelGGL(cross_values_kernel, dim3((unsigned)((pairs + 63) / 64), (unsigned)((nS + 63) / 64)), dim3(kCrossBlock), 0, h->stream, vio);
        HIP_TRY(h, hipGetLastError());
        if (length) HIP_TRY(h, hipMemcpyAsync(length + first, own.length, (size_t)pairs * 8, hipMemcpyDeviceToHost, h->stream));
        if (sums) HIP_TRY(h, hipMemcpyAsync(expect + (size_t)first * sums, own.expect, (size_t)pairs * sums * 8, hipMemcpyDeviceToHost, h->stream));
        if (iterations) HIP_TRY(h, hipMemcpyAsync(iterations + first, F.iter, (size_t)pairs * 4, hipMemcpyDeviceToHost, h->stream));
        if (occupancy) HIP_TRY(h, hipMemcpyAsync(occupancy + (size_t)first * nS, F.values, (size_t)pairs * nS * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return SOCCER_OK;
    });
}

// ------------------------------------------------------------------------------------------------
// exact policy gradients: for every pair cross-play's V and the occupancy's D with the discount as the continuation
// probability, solved pass by pass over the same pairs at one stride (hence a family of its own), one more backup from every
// pair's final V mixed with the other side's policy (action_values_kernel), and D * Q added to each policy's running weighted
// sum in ascending order of the other side's index (gradient_reduce_kernel), carried from pass to pass.

// a side's weights: finite, >= 0 and not all zero (NULL: every weight is 1.0 / n)
static int gradient_weights(soccer_handle* h, const char* what, const char* name, int n, const double* w, double* out) {
    bool any = false;
    for (int i = 0; i < n; ++i) {
        const double v = w ? w[i] : 1.0 / (double)n;
        if (!(v >= 0.0) || !(v <= DBL_MAX)) return fail(h, SOCCER_E_INVALID, "%s: %s[%d] is negative or not finite", what, name, i);
        any = any || v > 0.0;
        out[i] = v;
    }
    if (!any) return fail(h, SOCCER_E_INVALID, "%s: %s is all zero", what, name);
    return SOCCER_OK;
}

struct GradientOut {                        // HOST pointers, any may be NULL
    double* payoff; double* grad_a; double* grad_b; double* reach_a; double* reach_b;
    double* q_a; double* q_b; double* V; double* occupancy; int32_t* iterations;
};

// behind every check: pa / pb are [n][nS][5] where `kind` says (the caller's, or a learner's on the device), w is w_a then w_b.
// With `keep` the gradients are formed whatever is asked for and stay in h->gradient_own.grad (grad_a, then grad_b) for the caller.
static int gradient_solve(soccer_handle* h, const char* what, int n_a, const double* pa, int n_b, const double* pb, hipMemcpyKind kind,
                          double theta, double gamma, int32_t max_sweeps, int32_t pairs_per_pass, const std::vector<double>& w,
                          int normalize, bool keep, const GradientOut& out) {
    if (int rc = minimax_prepare(h)) return rc;
    if (int rc = build_occupancy_lists(h)) return rc;
    const int nS = h->mm.nS, total = n_a * n_b;
    const int per_pass = pass_pairs(pairs_per_pass, 112, nS, total);    // two V, two D and the ten action-value planes of a pass
    const bool grads = keep || out.grad_a || out.grad_b || out.reach_a || out.reach_b;
    const bool form_q = grads || out.q_a || out.q_b;
    PairBufs& F = h->gradient;
    GradientOwn& own = h->gradient_own;
    const size_t rows = (size_t)nS * 5;
    if (int rc = pair_buffers(h, F, {(size_t)nS, rows, true}, n_a + n_b, per_pass, out.q_a || out.q_b || out.V || out.occupancy,
                              [&](size_t policies, size_t stride) {
            own.D = F.pass;                                             // V's words and count: the two solves of a pass run one after the other
            own.D.stride = (int)stride;
            int rc = SOCCER_OK;
            for (int i = 0; i < 2 && !rc; ++i) rc = F.bufs.alloc(h, nS * stride, &own.D.buf[i]);
            if (!rc) rc = F.bufs.alloc(h, stride, &own.D.done);
            if (!rc) rc = F.bufs.alloc(h, 2 * rows * stride, &own.Q);
            if (!rc) rc = F.bufs.alloc(h, stride, &own.payoff);
            if (!rc) rc = F.bufs.alloc(h, policies * rows, &own.grad);
            if (!rc) rc = F.bufs.alloc(h, policies * nS, &own.reach);
            if (!rc) rc = F.bufs.alloc(h, policies, &own.w);
            return rc;
        })) return rc;
    const PassBufs& PV = F.pass; const PassBufs& PD = own.D;
    const int stride = PV.stride;
    double* d_grad_b = own.grad + (size_t)n_a * rows; double* d_reach_b = own.reach + (size_t)n_a * nS;
    double* d_Qa = own.Q; double* d_Qb = own.Q + rows * stride;
    if (int rc = pair_policies(h, F, n_a, pa, n_b, pb, kind)) return rc;
    if (grads) {
        HIP_TRY(h, hipMemcpyAsync(own.w, w.data(), (size_t)(n_a + n_b) * 8, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemsetAsync(own.grad, 0, (size_t)(n_a + n_b) * rows * 8, h->stream));     // every sum starts from 0.0
        HIP_TRY(h, hipMemsetAsync(own.reach, 0, (size_t)(n_a + n_b) * nS * 8, h->stream));
    }
    CrossIO cio = cross_io(h, F, n_a, n_b, gamma, theta);
    OccupancyIO oio = occupancy_io(h, F, n_a, n_b, gamma, theta);
    CrossFinishIO fio{};                                                // cross_finish_kernel's: the payoff
    fio.V[0] = PV.buf[0]; fio.V[1] = PV.buf[1]; fio.done_at = PV.done; fio.payoff = own.payoff; fio.iterations = F.iter;
    fio.values = F.values; fio.nS = nS; fio.stride = stride; fio.max_sweeps = max_sweeps;
    fill_isd(h, fio);
    CrossFinishIO dio = fio;                                            // cross_values_kernel's: D is laid out like V
    dio.V[0] = PD.buf[0]; dio.V[1] = PD.buf[1]; dio.done_at = PD.done;
    CrossFinishIO qio = fio;                                            // ... and a plane of action values like a V of nS * 5 rows
    qio.nS = (int32_t)rows;
    ActionValuesIO aio{};
    aio.offset = cio.offset; aio.list = cio.list; aio.x = cio.x; aio.y = cio.y; aio.V[0] = PV.buf[0]; aio.V[1] = PV.buf[1];
    aio.done_at = PV.done; aio.Qa = d_Qa; aio.Qb = d_Qb; aio.gamma = gamma; aio.nS = nS; aio.n_b = n_b; aio.stride = stride;
    aio.last = total - 1; aio.max_sweeps = max_sweeps;
    GradientReduceIO rio[2] = {};
    for (int side = 0; side < 2; ++side) {
        GradientReduceIO& r = rio[side];
        r.D[0] = PD.buf[0]; r.D[1] = PD.buf[1]; r.done_at = PD.done; r.Q = side ? d_Qb : d_Qa;
        r.w = own.w + (side ? 0 : n_a);                                 // the other side's
        r.grad = side ? d_grad_b : own.grad; r.reach = side ? d_reach_b : own.reach;
        r.side = side; r.n_a = n_a; r.n_b = n_b; r.nS = nS; r.stride = stride; r.max_sweeps = max_sweeps;
    }
    std::vector<int32_t> done((size_t)2 * per_pass);
    return pair_passes(h, what, total, per_pass, max_sweeps, [&](int first, int pairs, int32_t* open) -> int {
        const unsigned pair_waves = (unsigned)((pairs + 63) / 64);
        cio.first = first; cio.pairs = pairs; oio.first = first; oio.pairs = pairs;
        fio.pairs = pairs; dio.pairs = pairs; qio.pairs = pairs; aio.first = first; aio.pairs = pairs;
        // (the two counts of open pairs are not asked for: a pair is open if either solve is, which the stopping sweeps below tell)
        if (int rc = cross_solve_pass(h, cio, PV, max_sweeps, nullptr)) return rc;
        if (int rc = occupancy_solve_pass(h, oio, PD, max_sweeps, nullptr)) return rc;
        if (out.payoff) hipLaunchKernelGGL(cross_finish_kernel, dim3(pair_blocks(pairs)), dim3(kCrossBlock), 0, h->stream, fio);
        if (form_q)
            hipLaunchKernelGGL(action_values_kernel, dim3((unsigned)((nS + kCrossWaves - 1) / kCrossWaves), pair_waves), dim3(kCrossBlock), 0, h->stream, aio);
        for (int side = 0; side < 2 && grads; ++side) {
            rio[side].first = first; rio[side].pairs = pairs;
            const size_t threads = (size_t)(side ? n_b : n_a) * nS;
            hipLaunchKernelGGL(gradient_reduce_kernel, dim3((unsigned)((threads + kCrossBlock - 1) / kCrossBlock)), dim3(kCrossBlock), 0, h->stream, rio[side]);
        }
        HIP_TRY(h, hipGetLastError());
        if (out.payoff) HIP_TRY(h, hipMemcpyAsync(out.payoff + first, own.payoff, (size_t)pairs * 8, hipMemcpyDeviceToHost, h->stream));
        // V, D, q_a and q_b leave one after the other through the one transposed buffer (the stream keeps them in order)
        struct { double* dst; const CrossFinishIO* io; const double* plane; size_t width; } const leave[4] = {
            {out.V, &fio, nullptr, (size_t)nS}, {out.occupancy, &dio, nullptr, (size_t)nS}, {out.q_a, &qio, d_Qa, rows}, {out.q_b, &qio, d_Qb, rows}};
        for (const auto& l : leave) {
            if (!l.dst) continue;
            CrossFinishIO v = *l.io;
            if (l.plane) { v.V[0] = l.plane; v.V[1] = l.plane; }
            hipLaunchKernelGGL(cross_values_kernel, dim3(pair_waves, (unsigned)((l.width + 63) / 64)), dim3(kCrossBlock), 0, h->stream, v);
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, hipMemcpyAsync(l.dst + (size_t)first * l.width, F.values, (size_t)pairs * l.width * 8, hipMemcpyDeviceToHost, h->stream));
        }
        HIP_TRY(h, hipMemcpyAsync(done.data(), PV.done, (size_t)pairs * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemcpyAsync(done.data() + per_pass, PD.done, (size_t)pairs * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (int p = 0; p < pairs; ++p) {
            const int32_t kV = done[p], kD = done[(size_t)per_pass + p];
            if (!kV || !kD) *open += 1;
            if (out.iterations) {
                out.iterations[((size_t)first + p) * 2] = kV ? kV : max_sweeps;
                out.iterations[((size_t)first + p) * 2 + 1] = kD ? kD : max_sweeps;
            }
        }
        return SOCCER_OK;
    }, [&]() -> int {
        if (!grads) return SOCCER_OK;
        if (normalize) {
            GradientNormalizeIO nio{};
            nio.grad = own.grad; nio.reach = own.reach; nio.rows = (int64_t)(n_a + n_b) * nS;     // both sides: grad_b follows grad_a
            hipLaunchKernelGGL(gradient_normalize_kernel, dim3((unsigned)((nio.rows + kCrossBlock - 1) / kCrossBlock)), dim3(kCrossBlock), 0, h->stream, nio);
            HIP_TRY(h, hipGetLastError());
        }
        if (out.grad_a) HIP_TRY(h, hipMemcpyAsync(out.grad_a, own.grad, (size_t)n_a * rows * 8, hipMemcpyDeviceToHost, h->stream));
        if (out.grad_b) HIP_TRY(h, hipMemcpyAsync(out.grad_b, d_grad_b, (size_t)n_b * rows * 8, hipMemcpyDeviceToHost, h->stream));
        if (out.reach_a) HIP_TRY(h, hipMemcpyAsync(out.reach_a, own.reach, (size_t)n_a * nS * 8, hipMemcpyDeviceToHost, h->stream));
        if (out.reach_b) HIP_TRY(h, hipMemcpyAsync(out.reach_b, d_reach_b, (size_t)n_b * nS * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        return SOCCER_OK;
    });
}

extern "C" int soccer_policy_gradient(soccer_handle* h, int32_t n_a, const double* pi_a, int32_t n_b, const double* pi_b, double theta,
                                      double discount_factor, int32_t max_sweeps, int32_t pairs_per_pass, const double* w_a,
                                      const double* w_b, int32_t normalize, double* payoff, double* grad_a, double* grad_b,
                                      double* reach_a, double* reach_b, double* q_a, double* q_b, double* V, double* occupancy,
                                      int32_t* iterations) {
    const char* what = "soccer_policy_gradient";
    if (int rc = pair_check(h, what, "discount_factor", discount_factor, n_a, n_b, theta, max_sweeps, pairs_per_pass)) return rc;
    if (int rc = response_rows(h, what, "pi_a", n_a, pi_a)) return rc;
    if (int rc = response_rows(h, what, "pi_b", n_b, pi_b)) return rc;
    std::vector<double> w((size_t)n_a + n_b);
    if (int rc = gradient_weights(h, what, "w_a", n_a, w_a, w.data())) return rc;
    if (int rc = gradient_weights(h, what, "w_b", n_b, w_b, w.data() + n_a)) return rc;
    const GradientOut out{payoff, grad_a, grad_b, reach_a, reach_b, q_a, q_b, V, occupancy, iterations};
    return gradient_solve(h, what, n_a, pi_a, n_b, pi_b, hipMemcpyHostToDevice, theta, discount_factor, max_sweeps, pairs_per_pass, w,
                          normalize, false, out);
}

// ------------------------------------------------------------------------------------------------
// gradient play: both sets of policies live on the device and take projected steps along soccer_policy_gradient's
// gradients of themselves.  A learner is owned by the handle (its own list: it shares nothing with the sampled learners of
// soccer_learners.hip) and freed with it.
struct soccer_gradient_play {
    OwnedBufs bufs{"the gradient-play learner"};
    soccer_gradient_play_config cfg{};
    double* pol = nullptr;                  // [n_a + n_b][nS][5] x, then y
    double* prev = nullptr;                 // [n_a + n_b][nS][5] the previous step's gradients
    int64_t steps = 0;
    std::vector<double> w;                  // w_a, then w_b
    std::vector<double> payoff;             // [n_a][n_b] the last completed step's, before its update
};

void gradient_players_release(soccer_handle* h) {
    for (soccer_gradient_play* g : h->gradient_players) delete g;
    h->gradient_players.clear();
}

// the caller's pointer is only compared with the handle's list, never read
static int gradient_play_check(soccer_handle* h, const soccer_gradient_play* g, const char* what) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "%s during graph capture", what);
    if (!g || std::find(h->gradient_players.begin(), h->gradient_players.end(), g) == h->gradient_players.end())
        return fail(h, SOCCER_E_INVALID, "%s: not a gradient-play learner of this handle", what);
    return SOCCER_OK;
}

extern "C" int soccer_gradient_play_create(soccer_handle* h, const soccer_gradient_play_config* cfg, soccer_gradient_play** out) {
    const char* what = "soccer_gradient_play_create";
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (!cfg || !out) return fail(h, SOCCER_E_INVALID, "%s: cfg and out are required", what);
    *out = nullptr;
    if (int rc = pair_check(h, what, "discount_factor", cfg->discount_factor, cfg->n_a, cfg->n_b, cfg->theta, cfg->max_sweeps, cfg->pairs_per_pass)) return rc;
    if (!(cfg->eta_a >= 0.0 && cfg->eta_a <= DBL_MAX) || !(cfg->eta_b >= 0.0 && cfg->eta_b <= DBL_MAX))
        return fail(h, SOCCER_E_INVALID, "%s: eta_a and eta_b must be finite and >= 0", what);
    if (!(cfg->optimism >= 0.0 && cfg->optimism <= 1.0)) return fail(h, SOCCER_E_INVALID, "%s: optimism must be in [0, 1]", what);
    if (cfg->pi_a) if (int rc = response_rows(h, what, "pi_a", cfg->n_a, cfg->pi_a)) return rc;
    if (cfg->pi_b) if (int rc = response_rows(h, what, "pi_b", cfg->n_b, cfg->pi_b)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const int nS = h->rules.nS, n = cfg->n_a + cfg->n_b;
    const size_t rows = (size_t)nS * 5;
    soccer_gradient_play* g = new soccer_gradient_play();
    g->cfg = *cfg; g->cfg.pi_a = nullptr; g->cfg.pi_b = nullptr;
    g->w.resize((size_t)n); g->payoff.assign((size_t)cfg->n_a * cfg->n_b, 0.0);
    (void)gradient_weights(h, what, "w_a", cfg->n_a, nullptr, g->w.data());
    (void)gradient_weights(h, what, "w_b", cfg->n_b, nullptr, g->w.data() + cfg->n_a);
    int rc = g->bufs.alloc(h, (size_t)n * rows, &g->pol);
    if (!rc) rc = g->bufs.alloc(h, (size_t)n * rows, &g->prev);
    hipError_t e = hipSuccess;
    if (!rc) {
        const std::vector<double> uniform((size_t)std::max(cfg->n_a, cfg->n_b) * rows, 0.2);
        e = hipMemcpyAsync(g->pol, cfg->pi_a ? cfg->pi_a : uniform.data(), (size_t)cfg->n_a * rows * 8, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(g->pol + (size_t)cfg->n_a * rows, cfg->pi_b ? cfg->pi_b : uniform.data(), (size_t)cfg->n_b * rows * 8, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemsetAsync(g->prev, 0, (size_t)n * rows * 8, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) rc = fail(h, SOCCER_E_HIP, "%s failed: %s", what, hipGetErrorString(e));
    }
    if (rc) { delete g; return rc; }
    h->gradient_players.push_back(g);
    *out = g;
    return SOCCER_OK;
}

extern "C" int soccer_gradient_play_destroy(soccer_handle* h, soccer_gradient_play* g) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (!g) return SOCCER_OK;
    if (int rc = gradient_play_check(h, g, "soccer_gradient_play_destroy")) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // nothing is freed under a kernel that reads it
    h->gradient_players.erase(std::find(h->gradient_players.begin(), h->gradient_players.end(), g));
    delete g;
    return SOCCER_OK;
}

extern "C" int soccer_gradient_play_run(soccer_handle* h, soccer_gradient_play* g, int32_t n_steps, double* trace) {
    const char* what = "soccer_gradient_play_run";
    if (int rc = gradient_play_check(h, g, what)) return rc;
    if (n_steps < 0) return fail(h, SOCCER_E_INVALID, "%s: n_steps must be >= 0", what);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const soccer_gradient_play_config& c = g->cfg;
    const int nS = h->rules.nS;
    const size_t rows = (size_t)nS * 5, cells = (size_t)c.n_a * c.n_b;
    std::vector<double> payoff(cells);
    GradientOut out{};
    out.payoff = payoff.data();
    for (int32_t t = 0; t < n_steps; ++t) {
        // a step whose solves are still open is not applied: the state is that of the completed steps
        if (int rc = gradient_solve(h, what, c.n_a, g->pol, c.n_b, g->pol + (size_t)c.n_a * rows, hipMemcpyDeviceToDevice, c.theta,
                                    c.discount_factor, c.max_sweeps, c.pairs_per_pass, g->w, c.normalize, true, out)) return rc;
        GradientStepIO sio{};
        sio.pol = g->pol; sio.prev = g->prev; sio.grad = h->gradient_own.grad; sio.eta_a = c.eta_a; sio.eta_b = c.eta_b; sio.optimism = c.optimism;
        sio.rows_a = (int64_t)c.n_a * nS; sio.rows = (int64_t)(c.n_a + c.n_b) * nS; sio.nS = nS; sio.first_step = g->steps == 0;
        hipLaunchKernelGGL(gradient_step_kernel, dim3((unsigned)((sio.rows + kCrossBlock - 1) / kCrossBlock)), dim3(kCrossBlock), 0, h->stream, sio);
        HIP_TRY(h, hipGetLastError());
        g->payoff = payoff;
        if (trace) std::memcpy(trace + (size_t)t * cells, payoff.data(), cells * 8);
        g->steps += 1;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SOCCER_OK;
}

extern "C" int soccer_gradient_play_read(soccer_handle* h, soccer_gradient_play* g, double* pi_a, double* pi_b, double* prev_a,
                                         double* prev_b, double* w_a, double* w_b, double* payoff, int64_t* steps) {
    if (int rc = gradient_play_check(h, g, "soccer_gradient_play_read")) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t rows = (size_t)h->rules.nS * 5, na = (size_t)g->cfg.n_a * rows, nb = (size_t)g->cfg.n_b * rows;
    if (pi_a) HIP_TRY(h, hipMemcpyAsync(pi_a, g->pol, na * 8, hipMemcpyDeviceToHost, h->stream));
    if (pi_b) HIP_TRY(h, hipMemcpyAsync(pi_b, g->pol + na, nb * 8, hipMemcpyDeviceToHost, h->stream));
    if (prev_a) HIP_TRY(h, hipMemcpyAsync(prev_a, g->prev, na * 8, hipMemcpyDeviceToHost, h->stream));
    if (prev_b) HIP_TRY(h, hipMemcpyAsync(prev_b, g->prev + na, nb * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (w_a) std::memcpy(w_a, g->w.data(), (size_t)g->cfg.n_a * 8);
    if (w_b) std::memcpy(w_b, g->w.data() + g->cfg.n_a, (size_t)g->cfg.n_b * 8);
    if (payoff) std::memcpy(payoff, g->payoff.data(), g->payoff.size() * 8);
    if (steps) *steps = g->steps;
    return SOCCER_OK;
}

extern "C" int soccer_gradient_play_load(soccer_handle* h, soccer_gradient_play* g, const double* pi_a, const double* pi_b,
                                         const double* prev_a, const double* prev_b, const double* payoff, const int64_t* steps) {
    const char* what = "soccer_gradient_play_load";
    if (int rc = gradient_play_check(h, g, what)) return rc;
    if (pi_a) if (int rc = response_rows(h, what, "pi_a", g->cfg.n_a, pi_a)) return rc;
    if (pi_b) if (int rc = response_rows(h, what, "pi_b", g->cfg.n_b, pi_b)) return rc;
    if (steps && *steps < 0) return fail(h, SOCCER_E_INVALID, "%s: steps must be >= 0", what);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t rows = (size_t)h->rules.nS * 5, na = (size_t)g->cfg.n_a * rows, nb = (size_t)g->cfg.n_b * rows;
    if (pi_a) HIP_TRY(h, hipMemcpyAsync(g->pol, pi_a, na * 8, hipMemcpyHostToDevice, h->stream));
    if (pi_b) HIP_TRY(h, hipMemcpyAsync(g->pol + na, pi_b, nb * 8, hipMemcpyHostToDevice, h->stream));
    if (prev_a) HIP_TRY(h, hipMemcpyAsync(g->prev, prev_a, na * 8, hipMemcpyHostToDevice, h->stream));
    if (prev_b) HIP_TRY(h, hipMemcpyAsync(g->prev + na, prev_b, nb * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (payoff) std::memcpy(g->payoff.data(), payoff, g->payoff.size() * 8);
    if (steps) g->steps = *steps;
    return SOCCER_OK;
}

extern "C" int soccer_gradient_play_set_weights(soccer_handle* h, soccer_gradient_play* g, const double* w_a, const double* w_b) {
    const char* what = "soccer_gradient_play_set_weights";
    if (int rc = gradient_play_check(h, g, what)) return rc;
    std::vector<double> w(g->w.size());
    if (int rc = gradient_weights(h, what, "w_a", g->cfg.n_a, w_a, w.data())) return rc;
    if (int rc = gradient_weights(h, what, "w_b", g->cfg.n_b, w_b, w.data() + g->cfg.n_a)) return rc;
    g->w = w;
    return SOCCER_OK;
}
