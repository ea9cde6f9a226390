// soccer_planner_kernels.hpp — enumerate_kernel (the transition table), planner_kernel, the minimax kernels, response_sweep_kernel, minimax_lists_kernel, games_kernel.
// Included by soccer_planners.hip only: every kernel is emitted by exactly one translation unit.
#pragma once
#include "soccer_kernels.hpp"
#include "soccer_plan_io.hpp"
#include "soccer_simplex.hpp"

namespace soccer {

// =================================================================================================
// transition-table export: what the reference's constructor materialises as P_readable (:167-293)
// =================================================================================================
constexpr int kMaxOutcomes = 36;         // 9 slip combinations x up to 4 collision outcomes

struct EnumIO {
    int32_t* count;        // [n_tuples*25]   entries in the list, -1 for unreachable tuples (no key)
    double* prob;          // [n_tuples*25*36]
    int32_t* next;         // [n_tuples*25*36] flat tuple index of the next state
    int8_t* reward;        // [n_tuples*25*36] player A's reward
    uint8_t* done;         // [n_tuples*25*36]
    int32_t n_tuples, H;
};

// One thread per (state tuple, joint action): the ordered outcome list exactly as the reference builds
// it — combinations in order, zero weights dropped, collision outcomes in order, p = weight * outcome
// probability — using the same rule functions (moved / classify / pick) as the step kernels.
__global__ __launch_bounds__(kBlock) void enumerate_kernel(const KernelParams P, const EnumIO IO) {
    const long long gid = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= (long long)IO.n_tuples * 25) return;
    const int f = (int)(gid / 25), ja = (int)(gid % 25);
    const uint32_t aa = (uint32_t)(ja / 5), ab = (uint32_t)(ja % 5);
    int r = f;
    const uint32_t p = r & 1; r >>= 1;
    const uint32_t cb = r % P.W; r /= P.W;
    const uint32_t rb = r % IO.H; r /= IO.H;
    const uint32_t ca = r % P.W; const uint32_t ra = r / P.W;
    const uint32_t lut = P.lut[f];
    if (lut == 0xFFFFu) { IO.count[gid] = -1; return; }            // unreachable: the reference has no key (:179-180)
    Tables T; T.lut = P.lut; T.nc = P.next_cell; T.isd = P.isd;
    const uint32_t A = make_pos(ra, ca, P.W), B = make_pos(rb, cb, P.W);
    const bool in_goal = lut == 0u;                                  // goal tuple (:300-301)
    constexpr int VA[9] = {0, 0, 0, 1, 2, 1, 1, 2, 2};
    constexpr int VB[9] = {0, 1, 2, 0, 0, 1, 2, 1, 2};
    constexpr int CLS[9] = {0, 1, 1, 2, 2, 3, 3, 3, 3};
    const uint32_t Wm1 = (uint32_t)(P.W - 1);
    int n = 0;
    const long long base = gid * kMaxOutcomes;
    for (int c = 0; c < 9; ++c) {
        const double wgt = P.w[CLS[c]];
        if (wgt == 0.0) continue;                                    // :226-227
        if (in_goal) {                                               // absorbing self-loop, done, reward 0 (:235-236)
            IO.prob[base + n] = wgt * 1.0; IO.next[base + n] = f; IO.reward[base + n] = 0; IO.done[base + n] = 1; ++n;
            continue;
        }
        const uint32_t nA = moved(T, P, A, p ^ 1u, slip_move(aa, VA[c])), nB = moved(T, P, B, p, slip_move(ab, VB[c]));
        const Resolved R = classify(A, B, nA, nB, aa, ab);
        const int cnt = R.kind == K_COIN ? 2 : (R.kind == K_FOUR ? 4 : 1);
        const double q = cnt == 1 ? 1.0 : (cnt == 2 ? 0.5 : 0.25);
        for (int k = 0; k < cnt; ++k) {
            const Outcome o = pick(A, B, p, R, (uint32_t)k);
            const uint32_t ncc = col_of(o.p ? o.B : o.A);
            const bool goal = (ncc == 0u) | (ncc == Wm1);
            const int nf = (int)((((o.A >> 24) * (uint32_t)P.W + ((o.A >> 16) & 0xffu)) * (uint32_t)IO.H + (o.B >> 24)) * (uint32_t)P.W +
                                 ((o.B >> 16) & 0xffu)) * 2 + (int)o.p;
            IO.prob[base + n] = wgt * q;                             // :241
            IO.next[base + n] = nf;
            IO.reward[base + n] = goal ? (ncc == Wm1 ? 1 : -1) : 0;  // :237-240
            IO.done[base + n] = goal ? 1 : 0;
            ++n;
        }
    }
    IO.count[gid] = n;
}

// =================================================================================================
// planners on the single-agent transition lists (reference gym_soccer/utils/planners.py:4-87)
// =================================================================================================
// Q += prob * (reward + discount_factor * V[next_state] * (not done)), summed in list order (planners.py:12,28,39)
__device__ __forceinline__ double list_backup(const PlanIO& IO, const double* V, int s, int a) {
    double q = 0.0;
    const int end = IO.offset[s * 5 + a + 1];
    for (int e = IO.offset[s * 5 + a]; e < end; e += kPlanPad) {
        PlanEntry x[kPlanPad];
#pragma unroll
        for (int j = 0; j < kPlanPad; ++j) x[j] = IO.list[e + j];
#pragma unroll
        for (int j = 0; j < kPlanPad; ++j) {
            const double cont = (IO.gamma * V[x[j].next_done & 0x7fffffff]) * (x[j].next_done < 0 ? 0.0 : 1.0);
            q = q + x[j].prob * ((double)x[j].reward + cont);
        }
    }
    return q;
}

// dot(Pmat[s, :, a], v) with a sequential sum over the non-zero entries in ascending next-state index
__device__ __forceinline__ double dense_dot(const PlanIO& IO, const double* V, int s, int a) {
    double acc = 0.0;
    const int end = IO.m_offset[s * 5 + a + 1];
    for (int e = IO.m_offset[s * 5 + a]; e < end; e += kPlanPad) {
        PlanEntry x[kPlanPad];
#pragma unroll
        for (int j = 0; j < kPlanPad; ++j) x[j] = IO.m_list[e + j];
#pragma unroll
        for (int j = 0; j < kPlanPad; ++j) acc = acc + x[j].prob * V[x[j].next_done];
    }
    return acc;
}

// Rmat[s, a] + discount_factor * dot(Pmat[s, :, a], v)   (planners.py:62-65, :80)
__device__ __forceinline__ double dense_backup(const PlanIO& IO, const double* V, int s, int a) {
    return IO.m_R[s * 5 + a] + IO.gamma * dense_dot(IO, V, s, a);
}

// maximum of a non-negative double over the workgroup (such doubles order like their bit patterns)
__device__ __forceinline__ double block_max(double d, unsigned long long* slot) {
    if (threadIdx.x == 0) *slot = 0ull;
    __syncthreads();
    atomicMax(slot, (unsigned long long)__double_as_longlong(d));
    __syncthreads();
    const double r = __longlong_as_double((long long)*slot);
    __syncthreads();
    return r;
}

// One workgroup runs a whole planner: the problem is nS x 5 short lists, a launch per sweep would be pure
// launch latency.  Synchronous sweeps in float64 with V in LDS; the list-based planners (value iteration,
// policy evaluation / improvement / iteration) evaluate exactly the reference's expressions in the
// reference's order, so values, greedy policies and iteration counts are the reference's bit for bit;
// modified policy iteration follows the reference's dense Pmat/Rmat algebra with a sequential dot (numpy's
// BLAS dot associates differently: equal to ~1e-15 relative, see tests/test_planner.py).
__global__ __launch_bounds__(1024) void planner_kernel(const PlanIO IO) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    double* V = reinterpret_cast<double*>(smem);                 // [nS]
    __shared__ unsigned long long s_slot;
    const int nS = IO.nS, tid = threadIdx.x, nt = blockDim.x;
    int outer = 0, sweeps = 0, capped = 0;

    // greedy step over the lists: Q, first maximising action; returns max |V - max_a Q| over own states
    auto greedy_lists = [&](bool* changed) {
        double dmax = 0.0;
        for (int s = tid; s < nS; s += nt) {
            double best = 0.0; int arg = 0;
            for (int a = 0; a < 5; ++a) {
                const double q = list_backup(IO, V, s, a);
                IO.Q[s * 5 + a] = q;
                if (a == 0 || q > best) { best = q; arg = a; }            // np.argmax: first maximum
            }
            IO.newV[s] = best;
            if (changed && IO.pi[s] != arg) *changed = true;
            IO.pi[s] = arg;
            dmax = fmax(dmax, fabs(V[s] - best));
        }
        return dmax;
    };
    // policy_evaluation (planners.py:20-31) of IO.pi from zeros; leaves the result in IO.newV
    auto evaluate = [&]() {
        for (int s = tid; s < nS; s += nt) V[s] = 0.0;
        __syncthreads();
        for (;;) {
            double dmax = 0.0;
            for (int s = tid; s < nS; s += nt) {
                const double v = list_backup(IO, V, s, IO.pi[s]);
                IO.newV[s] = v;
                dmax = fmax(dmax, fabs(V[s] - v));
            }
            const double delta = block_max(dmax, &s_slot);
            ++sweeps;
            if (delta < IO.theta) break;
            if (sweeps >= IO.max_sweeps) { capped = 1; break; }
            for (int s = tid; s < nS; s += nt) V[s] = IO.newV[s];
            __syncthreads();
        }
    };

    if (IO.mode == kPlanVI) {                                   // planners.py:4-18
        for (int s = tid; s < nS; s += nt) V[s] = 0.0;
        __syncthreads();
        for (;;) {
            const double delta = block_max(greedy_lists(nullptr), &s_slot);
            ++outer; ++sweeps;
            if (delta < IO.theta) break;
            if (sweeps >= IO.max_sweeps) { capped = 1; break; }
            for (int s = tid; s < nS; s += nt) V[s] = IO.newV[s];
            __syncthreads();
        }
        for (int s = tid; s < nS; s += nt) IO.V[s] = V[s];       // the reference returns the pre-update V
    } else if (IO.mode == kPlanEval) {                          // planners.py:20-31
        evaluate();
        outer = sweeps;
        for (int s = tid; s < nS; s += nt) IO.V[s] = IO.newV[s];
    } else if (IO.mode == kPlanImprove) {                       // planners.py:33-41
        for (int s = tid; s < nS; s += nt) V[s] = IO.V[s];
        __syncthreads();
        (void)greedy_lists(nullptr);
        outer = 1;
    } else if (IO.mode == kPlanPI) {                            // planners.py:43-53
        for (;;) {
            evaluate();
            __syncthreads();
            for (int s = tid; s < nS; s += nt) { V[s] = IO.newV[s]; IO.V[s] = IO.newV[s]; }
            __syncthreads();
            bool changed = false;
            (void)greedy_lists(&changed);
            ++outer;
            const double any = block_max(changed ? 1.0 : 0.0, &s_slot);
            if (any == 0.0 || capped) break;
        }
    } else if (IO.mode == kPlanEvalDense) {                     // policy_eval, planners.py:55-70 (policy[s, a] in IO.Q)
        for (int s = tid; s < nS; s += nt) V[s] = IO.V[s];
        __syncthreads();
        for (int i = 0; i < IO.k; ++i) {
            double d2 = 0.0;
            for (int s = tid; s < nS; s += nt) {
                double r_pi = 0.0, p_pi = 0.0;
                for (int a = 0; a < 5; ++a) {
                    const double w = IO.Q[s * 5 + a];
                    const double acc = dense_dot(IO, V, s, a);
                    r_pi = r_pi + w * IO.m_R[s * 5 + a];
                    p_pi = p_pi + acc * w;
                }
                const double v = r_pi + IO.gamma * p_pi;
                IO.newV[s] = v;
                d2 = fmax(d2, fabs(v - V[s]));
            }
            const double delta = block_max(d2, &s_slot);
            for (int s = tid; s < nS; s += nt) V[s] = IO.newV[s];
            __syncthreads();
            ++sweeps;
            if (delta < IO.theta) break;
            if (sweeps >= IO.max_sweeps) { capped = 1; break; }
        }
        outer = sweeps;
        for (int s = tid; s < nS; s += nt) IO.V[s] = V[s];
    } else {                                                    // modified_policy_iteration, planners.py:73-87
        for (int s = tid; s < nS; s += nt) V[s] = 0.0;
        __syncthreads();
        for (;;) {
            double dmax = 0.0;
            for (int s = tid; s < nS; s += nt) {
                double best = 0.0; int arg = 0;
                for (int a = 0; a < 5; ++a) {
                    const double q = dense_backup(IO, V, s, a);
                    IO.Q[s * 5 + a] = q;
                    if (a == 0 || q > best) { best = q; arg = a; }
                }
                IO.newV[s] = best; IO.pi[s] = arg;
                dmax = fmax(dmax, fabs(V[s] - best));
            }
            const double gap = block_max(dmax, &s_slot);
            ++sweeps;
            if (gap <= IO.threshold) break;                       // returns greedy_v, q, counter (:83-84)
            if (sweeps >= IO.max_sweeps) { capped = 1; break; }
            for (int s = tid; s < nS; s += nt) V[s] = IO.newV[s];  // policy_eval(init = greedy_v), :55-70
            __syncthreads();
            for (int i = 0; i < IO.k; ++i) {
                double d2 = 0.0;
                for (int s = tid; s < nS; s += nt) {
                    const double v = dense_backup(IO, V, s, IO.pi[s]);
                    IO.newV[s] = v;
                    d2 = fmax(d2, fabs(v - V[s]));
                }
                const double delta = block_max(d2, &s_slot);
                for (int s = tid; s < nS; s += nt) V[s] = IO.newV[s];
                __syncthreads();
                ++sweeps;
                if (delta < IO.theta) break;
                if (sweeps >= IO.max_sweeps) { capped = 1; break; }
            }
            ++outer;
            if (capped) break;
        }
        for (int s = tid; s < nS; s += nt) IO.V[s] = IO.newV[s];
    }
    if (tid == 0) { IO.counters[0] = outer; IO.counters[1] = sweeps; IO.counters[2] = capped; }
}

// =================================================================================================
// minimax value iteration on the two-player lists (Shapley's operator; Littman 1994)
// =================================================================================================
// One launch is one synchronous (Jacobi) sweep over all states:
//   Q[s][a][b] = sum_k prob_k * (reward_k + (gamma * V[next_k]) * (done_k ? 0 : 1))   in list order, A's reward
//   V'[s]      = val(Q[s])   (soccer_games.hpp: saddle point exactly, else simplex with Bland's rule)
// A wave owns a state: lanes 0..24 gather the 25 joint actions' lists, lane 0 solves the stage game from LDS.  There is no
// grid-wide barrier: V is double-buffered across launches, max |V' - V| goes into a word of this sweep by atomicMax on the
// bit patterns of non-negative doubles, and a launch whose previous sweep's word is below theta returns at once — so the
// host can enqueue sweeps in batches and synchronise once per batch, and the result does not depend on the order in which
// workgroups run.
constexpr int kMinimaxBlock = 256;
constexpr int kMinimaxWaves = kMinimaxBlock / 64;

// the Q expression of list_backup, over the joint action's list
__device__ __forceinline__ double minimax_list_q(const MinimaxIO& IO, int key) {
    double q = 0.0;
    const int end = IO.offset[key + 1];
    for (int e = IO.offset[key]; e < end; e += kPlanPad) {
        PlanEntry x[kPlanPad];
#pragma unroll
        for (int j = 0; j < kPlanPad; ++j) x[j] = IO.list[e + j];
#pragma unroll
        for (int j = 0; j < kPlanPad; ++j) {
            const double cont = (IO.gamma * IO.V[x[j].next_done & 0x7fffffff]) * (x[j].next_done < 0 ? 0.0 : 1.0);
            q = q + x[j].prob * ((double)x[j].reward + cont);
        }
    }
    return q;
}

__global__ __launch_bounds__(kMinimaxBlock) void minimax_sweep_kernel(const MinimaxIO IO) {
    if (IO.prev && __longlong_as_double((long long)*IO.prev) < IO.theta) return;   // converged one sweep ago: nothing to do
    __shared__ double sQ[kMinimaxWaves][25];
    __shared__ GameWork sW[kMinimaxWaves];
    __shared__ unsigned long long s_max;
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const int s = (int)blockIdx.x * kMinimaxWaves + wave;
    if (threadIdx.x == 0) s_max = 0ull;
    if (s < IO.nS && lane < 25) {
        const double q = minimax_list_q(IO, s * 25 + lane);
        sQ[wave][lane] = q;
        IO.Q[(size_t)s * 25 + lane] = q;
    }
    __syncthreads();
    if (s < IO.nS && lane == 0) {
        double v = 0.0;
        solve_game5(sQ[wave], &sW[wave], &v, IO.pi_a ? IO.pi_a + (size_t)s * 5 : nullptr, IO.pi_b ? IO.pi_b + (size_t)s * 5 : nullptr);
        IO.V_out[s] = v;
        if (IO.delta) atomicMax(&s_max, (unsigned long long)__double_as_longlong(fabs(v - IO.V[s])));
    }
    __syncthreads();
    // a non-atomic look first: the word only grows, so a block whose maximum is not above what it sees has nothing to add
    if (IO.delta && threadIdx.x == 0 && s_max > *reinterpret_cast<volatile unsigned long long*>(IO.delta)) atomicMax(IO.delta, s_max);
}

// =================================================================================================
// best responses to mixed policies, and the value of a pair of them (soccer_best_response, soccer_evaluate_policies)
// =================================================================================================
// One launch is one synchronous sweep over all (policy, state) pairs, the policy in blockIdx.y, by minimax_sweep_kernel's
// scheme: V double-buffered per policy, max |V_k - V_{k-1}| by atomicMax into the policy's word of this sweep, and a block
// whose policy's previous word is below theta returns at once — a policy that has converged keeps the V, Qr and br of its
// own last sweep while the others go on, and solves to the bits it gives alone.  Half a wave owns a state (lanes 0..24 and
// 32..56): its 25 lanes gather the joint actions' lists into LDS, five of them form the five mixed sums in index order
// (acc = acc + p[i] * q[i] from 0.0, not contracted), its first lane takes the first minimum / maximum, or the outer sum.
constexpr int kResponseStates = 2 * kMinimaxWaves;      // states per workgroup

template <int MODE>
__global__ __launch_bounds__(kMinimaxBlock) void response_sweep_kernel(const ResponseIO IO) {
    const size_t pol = blockIdx.y;
    if (__longlong_as_double((long long)IO.prev[pol * (size_t)IO.word_stride]) < IO.mm.theta) return;   // this policy converged earlier
    __shared__ double sQ[kResponseStates][25];
    __shared__ double sR[kResponseStates][5];
    __shared__ unsigned long long s_max;
    const int slot = (int)(threadIdx.x >> 5), lane = (int)(threadIdx.x & 31u);
    const int nS = IO.mm.nS;
    const int s = (int)blockIdx.x * kResponseStates + slot;
    const size_t row = pol * (size_t)nS + (size_t)(s < nS ? s : 0);
    MinimaxIO M = IO.mm;
    M.V = IO.V + pol * (size_t)nS;
    if (threadIdx.x == 0) s_max = 0ull;
    if (s < nS && lane < 25) sQ[slot][lane] = minimax_list_q(M, s * 25 + lane);
    __syncthreads();
    if (s < nS && lane < 5) {
        // the fixed side's row; the lane's index belongs to the side that answers (kEvalPair: to A, the inner sum is over B's)
        const double* p = (MODE == kRespondB ? IO.x : IO.y) + row * 5;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < 5; ++i) acc = acc + p[i] * (MODE == kRespondB ? sQ[slot][i * 5 + lane] : sQ[slot][lane * 5 + i]);
        sR[slot][lane] = acc;
        if (MODE != kEvalPair) IO.Qr[row * 5 + lane] = acc;
    }
    __syncthreads();
    if (s < nS && lane == 0) {
        double v = 0.0;
        if (MODE == kEvalPair) {
            const double* p = IO.x + row * 5;
#pragma unroll
            for (int i = 0; i < 5; ++i) v = v + p[i] * sR[slot][i];
        } else {
            int arg = 0;
            v = sR[slot][0];
#pragma unroll
            for (int i = 1; i < 5; ++i) {
                const double r = sR[slot][i];
                if (MODE == kRespondB ? r < v : r > v) { v = r; arg = i; }       // the first index that attains it
            }
            IO.br[row] = arg;
        }
        IO.V_out[row] = v;
        atomicMax(&s_max, (unsigned long long)__double_as_longlong(fabs(v - M.V[s])));
    }
    __syncthreads();
    unsigned long long* word = IO.delta + pol * (size_t)IO.word_stride;
    if (threadIdx.x == 0 && s_max > *reinterpret_cast<volatile unsigned long long*>(word)) atomicMax(word, s_max);
}

// the two-player lists assembled on the device from enumerate_kernel's output (build_minimax): a thread per (state, joint
// action).  Pass 1 writes each list's padded length to offset[key + 1]; the host turns them into offsets; pass 2 copies the
// entries in enumeration order and pads — the lists the host would assemble, entry for entry.
struct MinimaxListIO {
    const int32_t* count; const double* prob; const int32_t* next; const int8_t* reward; const uint8_t* done;   // EnumIO's
    const int32_t* tuple_of;         // [nS] the tuple whose lists observation index s owns (index 0: the last goal tuple)
    const uint16_t* lut;             // observation index of a tuple (goal tuples: 0)
    int32_t* offset; PlanEntry* list;
    int32_t nS;
};
template <bool SCATTER>
__global__ __launch_bounds__(kBlock) void minimax_lists_kernel(const MinimaxListIO IO) {
    const long long key = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (key >= (long long)IO.nS * 25) return;
    const long long src = (long long)IO.tuple_of[key / 25] * 25 + key % 25;
    const int n = IO.count[src] > 0 ? IO.count[src] : 0;
    if (!SCATTER) { IO.offset[key + 1] = (n + kPlanPad - 1) / kPlanPad * kPlanPad; return; }
    int e = IO.offset[key];
    const int end = IO.offset[key + 1];
    for (int k = 0; k < n; ++k, ++e) {
        const long long x = src * kMaxOutcomes + k;
        IO.list[e] = PlanEntry{IO.prob[x], (int32_t)IO.lut[IO.next[x]] | (IO.done[x] ? (int32_t)0x80000000 : 0), (float)IO.reward[x]};
    }
    for (; e < end; ++e) IO.list[e] = PlanEntry{0.0, (int32_t)0x80000000, 0.0f};
}

// n independent games, a thread per game (soccer_solve_matrix_games)
constexpr int kGamesBlock = 64;
__global__ __launch_bounds__(kGamesBlock) void games_kernel(const double* A, long long n, double* value, double* x, double* y) {
    __shared__ GameWork sW[kGamesBlock];
    const long long g = (long long)blockIdx.x * kGamesBlock + threadIdx.x;
    if (g >= n) return;
    double v = 0.0;
    solve_game5(A + g * 25, &sW[threadIdx.x], &v, x ? x + g * 5 : nullptr, y ? y + g * 5 : nullptr);
    if (value) value[g] = v;
}

}  // namespace soccer
