// soccer_pair_kernels.hpp — the kernels of the pair evaluators: the cross-play kernels, the match-outcome kernels, the occupancy kernels, the policy-gradient kernels and gradient play's step.
// Included by soccer_pairs.hip only: every kernel is emitted by exactly one translation unit.
#pragma once
#include "soccer_kernels.hpp"
#include "soccer_plan_io.hpp"
#include "soccer_simplex.hpp"

namespace soccer {

// =================================================================================================
// the payoff matrix of n_a x n_b mixed policies (soccer_cross_play)
// =================================================================================================
// Pair (i, j) is kEvalPair's iteration on (x_i, y_j), the same sums in the same order, by minimax_sweep_kernel's scheme (a
// launch per sweep, V double-buffered, a word per pair and sweep) — with the work transposed: a lane owns a pair and a wave
// owns (state, 64 consecutive pairs of the pass).  The state is wave-uniform, so the list offsets and entries sit at
// wave-uniform addresses (scalar loads, one fetch per wave), and with V laid out [nS][stride] the 64 lanes' V[next] are one
// contiguous 512-byte load.  Padding entries are accumulated like any other.  The waves of a workgroup share their 64 pairs
// and take consecutive states; a pair whose previous word is below theta (and a lane past the end of a ragged pass) writes
// neither V nor its word, and the workgroup returns at once when that holds for all 64.
constexpr int kCrossBlock = 256;
constexpr int kCrossWaves = kCrossBlock / 64;

__global__ __launch_bounds__(kCrossBlock) void cross_sweep_kernel(const CrossIO IO) {
    __shared__ unsigned long long sD[kCrossWaves][64];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int p = (int)blockIdx.y * 64 + lane;
    const bool live = p < IO.pairs && !(__longlong_as_double((long long)IO.prev[p]) < IO.theta);
    if (__ballot(live) == 0ull) return;                                 // the same in every wave: they share the 64 pairs
    const int s = (int)blockIdx.x * kCrossWaves + wave;                 // wave-uniform, and so is every list index below
    const size_t stride = (size_t)IO.stride;
    unsigned long long d = 0ull;
    if (s < IO.nS) {
        const int g = min(IO.first + p, IO.last);                       // (a lane past the end reads the last pair's rows)
        const int i = g / IO.n_b, j = g - i * IO.n_b;
        const double* xr = IO.x + ((size_t)i * IO.nS + s) * 5;
        const double* yr = IO.y + ((size_t)j * IO.nS + s) * 5;
        const double* Vp = IO.V + p;
        double v = 0.0;
#pragma unroll 1
        for (int a = 0; a < 5; ++a) {
            const double xa = xr[a];                                    // (asked for before the lists that hide its latency)
            double inner = 0.0;
#pragma unroll 1
            for (int b = 0; b < 5; ++b) {
                const double yb = yr[b];
                const int key = s * 25 + a * 5 + b;
                const int end = IO.offset[key + 1];
                double q = 0.0;                                         // minimax_list_q's expression
                for (int e = IO.offset[key]; e < end; e += kPlanPad) {
                    PlanEntry x[kPlanPad];
                    double vn[kPlanPad];
#pragma unroll
                    for (int t = 0; t < kPlanPad; ++t) x[t] = IO.list[e + t];
#pragma unroll
                    for (int t = 0; t < kPlanPad; ++t) vn[t] = Vp[(size_t)(x[t].next_done & 0x7fffffff) * stride];
#pragma unroll
                    for (int t = 0; t < kPlanPad; ++t) {
                        const double cont = (IO.gamma * vn[t]) * (x[t].next_done < 0 ? 0.0 : 1.0);
                        q = q + x[t].prob * ((double)x[t].reward + cont);
                    }
                }
                inner = inner + yb * q;
            }
            v = v + xa * inner;
        }
        if (live) {
            IO.V_out[(size_t)s * stride + p] = v;
            d = (unsigned long long)__double_as_longlong(fabs(v - Vp[(size_t)s * stride]));
        }
    }
    sD[wave][lane] = d;
    __syncthreads();
    if (wave == 0 && live) {
#pragma unroll
        for (int w = 1; w < kCrossWaves; ++w) d = max(d, sD[w][lane]);
        // a non-atomic look first: the word only grows
        if (d > *reinterpret_cast<volatile unsigned long long*>(IO.delta + p)) atomicMax(IO.delta + p, d);
    }
}

// a thread per pair of the pass, between two batches of sweeps: the first sweep of the batch whose word is below theta is
// the pair's stopping sweep; row 0 takes the batch's last word (a pair that has stopped keeps a word below theta), the
// other rows are cleared for the next batch
__global__ __launch_bounds__(kCrossBlock) void cross_batch_kernel(const CrossBatchIO IO) {
    const int p = (int)blockIdx.x * kCrossBlock + (int)threadIdx.x;
    if (p >= IO.pairs) return;
    int done = IO.nb ? IO.done_at[p] : 0;
    for (int j = 1; j <= IO.nb; ++j)
        if (!done && __longlong_as_double((long long)IO.words[(size_t)j * IO.stride + p]) < IO.theta) done = IO.k0 + j - 1;
    IO.done_at[p] = done;
    IO.words[p] = IO.nb ? IO.words[(size_t)IO.nb * IO.stride + p] : (unsigned long long)__double_as_longlong(__builtin_huge_val());
    for (int j = 1; j < IO.n_words; ++j) IO.words[(size_t)j * IO.stride + p] = 0ull;
    if (!done) atomicAdd(IO.open, 1);
}

// a thread per pair: the sweep count (max_sweeps for an open pair) and player A's value at kick-off, from the buffer of the
// pair's own parity
__global__ __launch_bounds__(kCrossBlock) void cross_finish_kernel(const CrossFinishIO IO) {
    const int p = (int)blockIdx.x * kCrossBlock + (int)threadIdx.x;
    if (p >= IO.pairs) return;
    const int k = IO.done_at[p] ? IO.done_at[p] : IO.max_sweeps;
    const double* V = IO.V[k & 1] + p;
    double sum = 0.0;
    for (int i = 0; i < IO.n_isd; ++i) sum = sum + V[(size_t)IO.isd[i] * IO.stride];
    IO.payoff[p] = sum / (double)IO.n_isd;
    IO.iterations[p] = k;
}

// V[nS][stride] -> values[pair][nS] through a 64 x 64 tile in LDS, both sides coalesced
__global__ __launch_bounds__(kCrossBlock) void cross_values_kernel(const CrossFinishIO IO) {
    __shared__ double tile[64][65];
    const int col = (int)(threadIdx.x & 63u), row0 = (int)(threadIdx.x >> 6);
    const int p0 = (int)blockIdx.x * 64, s0 = (int)blockIdx.y * 64;
    {
        const int p = p0 + col;
        const int k = p < IO.pairs ? (IO.done_at[p] ? IO.done_at[p] : IO.max_sweeps) : 0;
        const double* V = IO.V[k & 1] + p;
        for (int r = row0; r < 64; r += kCrossWaves)
            if (p < IO.pairs && s0 + r < IO.nS) tile[r][col] = V[(size_t)(s0 + r) * IO.stride];
    }
    __syncthreads();
    for (int r = row0; r < 64; r += kCrossWaves)
        if (p0 + r < IO.pairs && s0 + col < IO.nS) IO.values[(size_t)(p0 + r) * IO.nS + s0 + col] = tile[col][r];
}

// =================================================================================================
// match outcomes of n_a x n_b mixed policies (soccer_match_outcomes)
// =================================================================================================
// cross_sweep_kernel's work layout, scheme and stopping, with three value vectors per pair instead of one: W_A (A scores the
// goal that ends the game), W_B (B does) and L (the steps the game lasts).  A list entry is fetched once, by scalar loads, and
// feeds all three accumulators; the two goal indicators are wave-uniform like the entry they come from.  The V buffers are
// laid out [nS][3][stride]: a channel's V[next] of the 64 lanes is one contiguous 512-byte load as in cross-play, and the
// three loads of an entry are 8 * stride bytes apart, rows of one block, where [3][nS][stride] would put them nS * stride * 8
// bytes apart.  IO is a CrossIO whose V and V_out have that layout and whose gamma is the continuation probability; one word
// per pair and sweep carries the maximum over the three channels, so cross_batch_kernel serves unchanged.
constexpr int kMatchChannels = 3;

__global__ __launch_bounds__(kCrossBlock) void match_sweep_kernel(const CrossIO IO) {
    __shared__ unsigned long long sD[kCrossWaves][64];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int p = (int)blockIdx.y * 64 + lane;
    const bool live = p < IO.pairs && !(__longlong_as_double((long long)IO.prev[p]) < IO.theta);
    if (__ballot(live) == 0ull) return;                                 // the same in every wave: they share the 64 pairs
    const int s = (int)blockIdx.x * kCrossWaves + wave;                 // wave-uniform, and so is every list index below
    const size_t stride = (size_t)IO.stride;
    unsigned long long d = 0ull;
    if (s < IO.nS) {
        const int g = min(IO.first + p, IO.last);                       // (a lane past the end reads the last pair's rows)
        const int i = g / IO.n_b, j = g - i * IO.n_b;
        const double* xr = IO.x + ((size_t)i * IO.nS + s) * 5;
        const double* yr = IO.y + ((size_t)j * IO.nS + s) * 5;
        const double* Vp = IO.V + p;
        double vA = 0.0, vB = 0.0, vL = 0.0;
#pragma unroll 1
        for (int a = 0; a < 5; ++a) {
            const double xa = xr[a];
            double iA = 0.0, iB = 0.0, iL = 0.0;
#pragma unroll 1
            for (int b = 0; b < 5; ++b) {
                const double yb = yr[b];
                const int key = s * 25 + a * 5 + b;
                const int end = IO.offset[key + 1];
                double qA = 0.0, qB = 0.0, qL = 0.0;                    // minimax_list_q's expression, three rewards
                for (int e = IO.offset[key]; e < end; e += kPlanPad) {
                    PlanEntry x[kPlanPad];
                    double fA[kPlanPad], fB[kPlanPad], fL[kPlanPad];
#pragma unroll
                    for (int t = 0; t < kPlanPad; ++t) x[t] = IO.list[e + t];
#pragma unroll
                    for (int t = 0; t < kPlanPad; ++t) {
                        const double* row = Vp + (size_t)(x[t].next_done & 0x7fffffff) * (kMatchChannels * stride);
                        fA[t] = row[0]; fB[t] = row[stride]; fL[t] = row[2 * stride];
                    }
#pragma unroll
                    for (int t = 0; t < kPlanPad; ++t) {
                        const double go = x[t].next_done < 0 ? 0.0 : 1.0;
                        qA = qA + x[t].prob * ((x[t].reward > 0.0f ? 1.0 : 0.0) + (IO.gamma * fA[t]) * go);
                        qB = qB + x[t].prob * ((x[t].reward < 0.0f ? 1.0 : 0.0) + (IO.gamma * fB[t]) * go);
                        qL = qL + x[t].prob * (1.0 + (IO.gamma * fL[t]) * go);
                    }
                }
                iA = iA + yb * qA; iB = iB + yb * qB; iL = iL + yb * qL;
            }
            vA = vA + xa * iA; vB = vB + xa * iB; vL = vL + xa * iL;
        }
        if (live) {
            const size_t at = (size_t)s * (kMatchChannels * stride) + p;
            IO.V_out[at] = vA; IO.V_out[at + stride] = vB; IO.V_out[at + 2 * stride] = vL;
            const double* old = IO.V + at;
            // non-negative doubles order like their bit patterns
            d = (unsigned long long)__double_as_longlong(fabs(vA - old[0]));
            d = max(d, (unsigned long long)__double_as_longlong(fabs(vB - old[stride])));
            d = max(d, (unsigned long long)__double_as_longlong(fabs(vL - old[2 * stride])));
        }
    }
    sD[wave][lane] = d;
    __syncthreads();
    if (wave == 0 && live) {
#pragma unroll
        for (int w = 1; w < kCrossWaves; ++w) d = max(d, sD[w][lane]);
        // a non-atomic look first: the word only grows
        if (d > *reinterpret_cast<volatile unsigned long long*>(IO.delta + p)) atomicMax(IO.delta + p, d);
    }
}

// a thread per pair: the sweep count (max_sweeps for an open pair) and the three kick-off means, from the buffer of the pair's
// own parity
__global__ __launch_bounds__(kCrossBlock) void match_finish_kernel(const MatchFinishIO IO) {
    const int p = (int)blockIdx.x * kCrossBlock + (int)threadIdx.x;
    if (p >= IO.pairs) return;
    const int k = IO.done_at[p] ? IO.done_at[p] : IO.max_sweeps;
    const size_t stride = (size_t)IO.stride;
    for (int c = 0; c < kMatchChannels; ++c) {
        const double* V = IO.V[k & 1] + (size_t)c * stride + p;
        double sum = 0.0;
        for (int i = 0; i < IO.n_isd; ++i) sum = sum + V[(size_t)IO.isd[i] * (kMatchChannels * stride)];
        IO.kickoff[(size_t)c * stride + p] = sum / (double)IO.n_isd;
    }
    IO.iterations[p] = k;
}

// V[nS][3][stride] -> values[pair][3][nS]: cross_values_kernel's 64 x 64 tile in LDS, the channel in blockIdx.z
__global__ __launch_bounds__(kCrossBlock) void match_values_kernel(const MatchFinishIO IO) {
    __shared__ double tile[64][65];
    const int col = (int)(threadIdx.x & 63u), row0 = (int)(threadIdx.x >> 6);
    const int p0 = (int)blockIdx.x * 64, s0 = (int)blockIdx.y * 64, c = (int)blockIdx.z;
    const size_t stride = (size_t)IO.stride;
    {
        const int p = p0 + col;
        const int k = p < IO.pairs ? (IO.done_at[p] ? IO.done_at[p] : IO.max_sweeps) : 0;
        const double* V = IO.V[k & 1] + (size_t)c * stride + p;
        for (int r = row0; r < 64; r += kCrossWaves)
            if (p < IO.pairs && s0 + r < IO.nS) tile[r][col] = V[(size_t)(s0 + r) * (kMatchChannels * stride)];
    }
    __syncthreads();
    for (int r = row0; r < 64; r += kCrossWaves)
        if (p0 + r < IO.pairs && s0 + col < IO.nS)
            IO.values[((size_t)(p0 + r) * kMatchChannels + c) * IO.nS + s0 + col] = tile[col][r];
}

// =================================================================================================
// state occupancy of n_a x n_b mixed policies (soccer_occupancy)
// =================================================================================================
// The dual of cross-play's evaluation: D_k[s'] = mu[s'] + sum over the in-entries of s' of prob * ((x[s][a] * y[s][b]) *
// (c * D_{k-1}[s])), the transition relation run backwards.  A gather over in-lists (soccer_inlists.hpp) rather than a
// scatter along the out-lists, so every D_k[s'] is one sequential sum in one fixed order and needs no atomics.
// cross_sweep_kernel's work layout, scheme and stopping: a lane owns a pair, a wave owns (s', 64 consecutive pairs of the
// pass), D is [nS][stride], the in-entries sit at wave-uniform addresses (scalar loads, kPlanPad per wait) and an entry's
// D[s] of the 64 lanes is one contiguous 512-byte load.  New here: the policy entries are read per in-entry, at that entry's
// (s, a) and (s, b), not once per state.  They come from transposed copies [nS][5][n] (occupancy_transpose_kernel), so the
// 64 lanes' y[s][b][j] are consecutive doubles (j = pair mod n_b) and their x[s][a][i] one or two addresses, where the
// caller's [n][nS][5] would put each lane's y in a cache line of its own, nS * 40 bytes from its neighbour's.  Row 0 of D is
// never written and stays 0.0; a padding in-entry (key 0) reads the zeroed row 0 of both policies and adds +0.0.
__global__ __launch_bounds__(kCrossBlock) void occupancy_transpose_kernel(const OccupancyPolicyIO IO) {
    const size_t at = (size_t)blockIdx.x * kCrossBlock + threadIdx.x;
    if (at >= (size_t)IO.rows * (size_t)IO.n) return;
    const size_t r = at / (size_t)IO.n, i = at - r * (size_t)IO.n;
    IO.polT[at] = r < 5 ? 0.0 : IO.pol[i * (size_t)IO.rows + r];
}

__global__ __launch_bounds__(kCrossBlock) void occupancy_sweep_kernel(const OccupancyIO IO) {
    __shared__ unsigned long long sD[kCrossWaves][64];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int p = (int)blockIdx.y * 64 + lane;
    const bool live = p < IO.pairs && !(__longlong_as_double((long long)IO.prev[p]) < IO.theta);
    if (__ballot(live) == 0ull) return;                                 // the same in every wave: they share the 64 pairs
    const int s1 = (int)blockIdx.x * kCrossWaves + wave;                // s': wave-uniform, and so is every in-list index below
    const size_t stride = (size_t)IO.stride;
    unsigned long long d = 0ull;
    if (s1 >= 1 && s1 < IO.nS) {
        const int g = min(IO.first + p, IO.last);                       // (a lane past the end reads the last pair's rows)
        const int i = g / IO.n_b, j = g - i * IO.n_b;
        const double* xp = IO.xT + i;
        const double* yp = IO.yT + j;
        const double* Dp = IO.D + p;
        double mu = 0.0;
        for (int t = 0; t < IO.n_isd; ++t) mu = IO.isd[t] == s1 ? IO.mu : mu;
        const int end = IO.in_offset[s1 + 1];
        double acc = 0.0;
        for (int e = IO.in_offset[s1]; e < end; e += kPlanPad) {
            InEntry x[kPlanPad];
            double xa[kPlanPad], yb[kPlanPad], ds[kPlanPad];
#pragma unroll
            for (int t = 0; t < kPlanPad; ++t) x[t] = IO.in_list[e + t];
#pragma unroll
            for (int t = 0; t < kPlanPad; ++t) {
                const int key = x[t].source_key, s = key / 25;         // key = s * 25 + a * 5 + b
                xa[t] = xp[(size_t)(key / 5) * (size_t)IO.n_a];                            // x[s][a]
                yb[t] = yp[(size_t)(s * 5 + (key - (key / 5) * 5)) * (size_t)IO.n_b];      // y[s][b]
                ds[t] = Dp[(size_t)s * stride];
            }
#pragma unroll
            for (int t = 0; t < kPlanPad; ++t) acc = acc + x[t].prob * ((xa[t] * yb[t]) * (IO.c * ds[t]));
        }
        if (live) {
            const double v = mu + acc;
            IO.D_out[(size_t)s1 * stride + p] = v;
            d = (unsigned long long)__double_as_longlong(fabs(v - Dp[(size_t)s1 * stride]));   // non-negative doubles order like their bits
        }
    }
    sD[wave][lane] = d;
    __syncthreads();
    if (wave == 0 && live) {
#pragma unroll
        for (int w = 1; w < kCrossWaves; ++w) d = max(d, sD[w][lane]);
        // a non-atomic look first: the word only grows
        if (d > *reinterpret_cast<volatile unsigned long long*>(IO.delta + p)) atomicMax(IO.delta + p, d);
    }
}

// a thread per (pair, sum), the sum in blockIdx.y: 0 is the sweep count (max_sweeps for an open pair) and, if asked for, the
// length sum_s D[s]; q >= 1 the expectation sum_s D[s] * features[q - 1][s].  Each sum is sequential over ascending s from
// 0.0, from the buffer of the pair's own parity; the 64 lanes' D[s] are one contiguous load and the feature is wave-uniform.
__global__ __launch_bounds__(kCrossBlock) void occupancy_finish_kernel(const OccupancyFinishIO IO) {
    const int p = (int)blockIdx.x * kCrossBlock + (int)threadIdx.x;
    const int q = (int)blockIdx.y;
    if (p >= IO.pairs) return;
    const int k = IO.done_at[p] ? IO.done_at[p] : IO.max_sweeps;
    if (q == 0) {
        IO.iterations[p] = k;
        if (!IO.length) return;
    }
    const double* D = IO.D[k & 1] + p;
    const size_t stride = (size_t)IO.stride;
    double sum = 0.0;
    if (q == 0) {
        for (int s = 0; s < IO.nS; ++s) sum = sum + D[(size_t)s * stride];
        IO.length[p] = sum;
    } else {
        const double* f = IO.features + (size_t)(q - 1) * IO.nS;
        for (int s = 0; s < IO.nS; ++s) sum = sum + D[(size_t)s * stride] * f[s];
        IO.expect[(size_t)p * IO.n_f + (q - 1)] = sum;
    }
}

// =================================================================================================
// exact policy gradients of n_a x n_b mixed policies (soccer_policy_gradient), and gradient play on them
// =================================================================================================
// After a pass's V and D have stopped: one more backup from every pair's final V, q[a][b] = minimax_list_q's expression
// (padding entries accumulated), mixed with the other side's policy — Q_a[s][a] = sum_b y[s][b] * q[a][b] over b = 0..4 from
// 0.0 and Q_b[s][b] = sum_a x[s][a] * q[a][b] over a = 0..4 from 0.0.  cross_sweep_kernel's layout: a lane owns a pair, a wave
// (state, 64 consecutive pairs), the list entries come by scalar loads, kPlanPad per wait, and an entry's V[next] of the 64
// lanes is one contiguous 512-byte load — from the buffer of each lane's own parity, a per-lane select of the base pointer as
// in cross_finish_kernel.  Q_a and Q_b are [nS][5][stride]: ten coalesced 512-byte stores per wave.  The loop over b is
// unrolled so that the five Q_b accumulators are named registers; the loop over a is not.
__device__ __forceinline__ double pair_list_q(const int32_t* offset, const PlanEntry* list, const double* Vp, size_t stride, double gamma, int key) {
    const int end = offset[key + 1];
    double q = 0.0;                                                     // minimax_list_q's expression
    for (int e = offset[key]; e < end; e += kPlanPad) {
        PlanEntry x[kPlanPad];
        double vn[kPlanPad];
#pragma unroll
        for (int t = 0; t < kPlanPad; ++t) x[t] = list[e + t];
#pragma unroll
        for (int t = 0; t < kPlanPad; ++t) vn[t] = Vp[(size_t)(x[t].next_done & 0x7fffffff) * stride];
#pragma unroll
        for (int t = 0; t < kPlanPad; ++t) {
            const double cont = (gamma * vn[t]) * (x[t].next_done < 0 ? 0.0 : 1.0);
            q = q + x[t].prob * ((double)x[t].reward + cont);
        }
    }
    return q;
}

__global__ __launch_bounds__(kCrossBlock) void action_values_kernel(const ActionValuesIO IO) {
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int p = (int)blockIdx.y * 64 + lane;                          // (< stride: a multiple of 64 that is >= pairs)
    const int s = (int)blockIdx.x * kCrossWaves + wave;                 // wave-uniform, and so is every list index below
    if (s >= IO.nS) return;
    const bool live = p < IO.pairs;
    const size_t stride = (size_t)IO.stride;
    int k = 0;
    if (live) k = IO.done_at[p] ? IO.done_at[p] : IO.max_sweeps;
    const double* Vp = ((k & 1) ? IO.V[1] : IO.V[0]) + p;               // (a lane past the end reads buffer 0: in bounds, not stored)
    const int g = min(IO.first + p, IO.last);                           // (... and the last pair's rows)
    const int i = g / IO.n_b, j = g - i * IO.n_b;
    const double* xr = IO.x + ((size_t)i * IO.nS + s) * 5;
    const double* yr = IO.y + ((size_t)j * IO.nS + s) * 5;
    double yb[5], qa[5], qb[5];
#pragma unroll
    for (int b = 0; b < 5; ++b) { yb[b] = yr[b]; qa[b] = 0.0; qb[b] = 0.0; }
    // Nothing is stored before the last list entry is read: a store inside the loop would let the compiler no longer prove
    // the lists unchanged, and it would fetch the entries by vector loads at a uniform address instead of scalar loads.
#pragma unroll 1
    for (int a = 0; a < 5; ++a) {
        const double xa = xr[a];
        double inner = 0.0;
#pragma unroll
        for (int b = 0; b < 5; ++b) {
            const double q = pair_list_q(IO.offset, IO.list, Vp, stride, IO.gamma, s * 25 + a * 5 + b);
            inner = inner + yb[b] * q;
            qb[b] = qb[b] + xa * q;
        }
#pragma unroll
        for (int c = 0; c < 5; ++c) qa[c] = c == a ? inner : qa[c];     // (a is wave-uniform: five selects, no indexed array)
    }
    if (live) {
#pragma unroll
        for (int c = 0; c < 5; ++c) IO.Qa[((size_t)s * 5 + c) * stride + p] = qa[c];
#pragma unroll
        for (int b = 0; b < 5; ++b) IO.Qb[((size_t)s * 5 + b) * stride + p] = qb[b];
    }
}

// a thread per (policy of this side, state): the pass's pairs of that policy's row (player A) or column (player B) of the
// matrix, in ascending order of the other side's index, added to the running reach and grad — reach = reach + w * D[s] and
// grad[a] = grad[a] + w * (D[s] * Q[s][a]).  The running values start as 0.0 (the host clears them once per call) and are
// carried from pass to pass, so a row that spans passes is one sequential sum.
__global__ __launch_bounds__(kCrossBlock) void gradient_reduce_kernel(const GradientReduceIO IO) {
    const size_t t = (size_t)blockIdx.x * kCrossBlock + threadIdx.x;
    const int n_own = IO.side ? IO.n_b : IO.n_a;
    if (t >= (size_t)n_own * (size_t)IO.nS) return;
    const int s = (int)(t / (size_t)n_own), own = (int)(t - (size_t)s * (size_t)n_own);
    // the other side's indices lo .. hi - 1 whose pair with `own` lies in this pass: matrix index g0 + o * step
    const long long first = IO.first, end = first + IO.pairs, nb = IO.n_b;
    long long g0, step, lo, hi;
    if (IO.side == 0) {
        g0 = (long long)own * nb; step = 1;
        lo = max(0ll, first - g0); hi = min(nb, end - g0);
    } else {
        g0 = own; step = nb;
        lo = first > g0 ? (first - g0 + nb - 1) / nb : 0ll;
        hi = end > g0 ? min((long long)IO.n_a, (end - 1 - g0) / nb + 1) : 0ll;
    }
    if (hi <= lo) return;
    const size_t stride = (size_t)IO.stride;
    double* gr = IO.grad + ((size_t)own * IO.nS + s) * 5;
    double* re = IO.reach + (size_t)own * IO.nS + s;
    double r = *re, g[5];
#pragma unroll
    for (int a = 0; a < 5; ++a) g[a] = gr[a];
    for (long long o = lo; o < hi; ++o) {
        const size_t p = (size_t)(g0 + o * step - first);
        const int k = IO.done_at[p] ? IO.done_at[p] : IO.max_sweeps;
        const double d = IO.D[k & 1][(size_t)s * stride + p];
        const double w = IO.w[o];
        r = r + w * d;
#pragma unroll
        for (int a = 0; a < 5; ++a) g[a] = g[a] + w * (d * IO.Q[((size_t)s * 5 + a) * stride + p]);
    }
    *re = r;
#pragma unroll
    for (int a = 0; a < 5; ++a) gr[a] = g[a];
}

__global__ __launch_bounds__(kCrossBlock) void gradient_normalize_kernel(const GradientNormalizeIO IO) {
    const size_t t = (size_t)blockIdx.x * kCrossBlock + threadIdx.x;
    if (t >= (size_t)IO.rows) return;
    const double r = IO.reach[t];
    double* g = IO.grad + t * 5;
#pragma unroll
    for (int a = 0; a < 5; ++a) g[a] = r > 0.0 ? g[a] / r : 0.0;
}

// a thread per row (policy, state) of both players: prev = g at the first step; d = g + optimism * (g - prev); prev = g; for
// every state but 0 the row becomes P(row + eta_a * d) (player A) or P(row - eta_b * d) (player B), P the projection of
// soccer_simplex.hpp.  Row 0 of a policy is never touched, and neither is any row of a side whose eta is 0.0.
__global__ __launch_bounds__(kCrossBlock) void gradient_step_kernel(const GradientStepIO IO) {
    const size_t t = (size_t)blockIdx.x * kCrossBlock + threadIdx.x;
    if (t >= (size_t)IO.rows) return;
    const bool is_a = t < (size_t)IO.rows_a;
    const size_t local = is_a ? t : t - (size_t)IO.rows_a;
    const bool row0 = local % (size_t)IO.nS == 0;
    const double* g = IO.grad + t * 5;
    double* pv = IO.prev + t * 5;
    double* pol = IO.pol + t * 5;
    double v[5], out[5];
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        const double ga = g[a];
        const double before = IO.first_step ? ga : pv[a];
        const double d = ga + IO.optimism * (ga - before);
        pv[a] = ga;
        v[a] = is_a ? pol[a] + IO.eta_a * d : pol[a] - IO.eta_b * d;
    }
    if (row0 || (is_a ? IO.eta_a : IO.eta_b) == 0.0) return;            // a side whose step is 0 is held fixed to the bit, not re-projected
    project_simplex5(v, out);
#pragma unroll
    for (int a = 0; a < 5; ++a) pol[a] = out[a];
}

}  // namespace soccer
