// soccer_learner_kernels.hpp — the minimax-Q learner (Littman 1994): learner_act_kernel, learner_reduce_kernel,
// learner_update_kernel, learner_init_kernel; and the independent Q-learners of both players: q_act_kernel, q_reduce_kernel,
// q_update_kernel, q_init_kernel (they share the act-and-step body, the reduce body and learner_thresholds); and the policy
// hill-climbers on top of those: phc_act_kernel, phc_reduce_kernel, phc_update_kernel, phc_init_kernel; and the regret
// matchers in the same shape: rm_act_kernel, rm_reduce_kernel, rm_update_kernel, rm_init_kernel; and the population
// of one-actor Q-learners, a learner per lane: pop_run_kernel, pop_league_run_kernel (against a league opponent),
// pop_update_kernel, pop_init_kernel; and the population of
// one-actor policy hill-climbers: phc_pop_run_kernel, phc_pop_update_kernel, phc_pop_init_kernel, phc_pop_adopt_kernel; and the
// population of one-actor minimax-Q learners, a wave per member: mq_pop_run_kernel, mq_pop_update_kernel, mq_pop_solve_kernel,
// mq_pop_init_kernel; and the population of one-actor opponent-modelling Q-learners: om_pop_run_kernel, om_pop_update_kernel,
// om_pop_init_kernel, om_pop_derive_kernel; and the population of one-actor regret matchers: rm_pop_run_kernel,
// rm_pop_update_kernel, rm_pop_init_kernel (at the end).
// Included by soccer_learners.hip only: every kernel is emitted by exactly one translation unit.
//
// One learner step (include/soccer_hip.h, "learners") is two launches in stream order, no grid barrier between them:
//   learner_act_kernel     every lane reads its observation s, draws both actions from the threshold rows the previous
//                          update left, takes the step of batched_rollout(n_steps = 1, sample_actions) — lane_step, the
//                          same Philox words, the same histogram — and adds its transition to the three INTEGER
//                          accumulators of its cell (count, reward sum, sum of Vq[s'])
//   learner_update_kernel  a wave per state, shaped like minimax_sweep_kernel: lanes 0..24 own the 25 cells, move the
//                          touched ones toward the mean target and zero the accumulators they read; a ballot says whether
//                          the state was touched; lane 0 solves the stage game from the wave's LDS slot and writes V, Vq,
//                          the strategies and the threshold rows of the next step; one thread advances alpha and the step
//                          counter.  alpha has two slots (read one, write the other, like the tick) because every wave
//                          of the launch reads it.
// Integer sums make the result independent of the order in which lanes arrive (float atomics would not be).
#pragma once
#include "soccer_kernels.hpp"
#include "soccer_league.hpp"

namespace soccer {

constexpr int kLearnerBlock = 256;
constexpr int kLearnerWaves = kLearnerBlock / 64;
constexpr double kVqScale = 0x1.0p40, kVqInv = 0x1.0p-40;     // the grid V is summed on

struct LearnerIO {
    double* Q;                          // [nS][25]
    double* V;                          // [nS]
    double* pi_a; double* pi_b;         // [nS][5]
    long long* Vq;                      // [nS] rint(V * 2^40)
    unsigned long long* visits;         // [nS][25]
    unsigned int* cnt;                  // [nS][25] samples of this step
    int* rsum;                          // [nS][25] sum of player A's rewards
    long long* sv;                      // [nS][25] sum of Vq[s'] over the non-terminated samples
    uint16_t* mix_a;                    // [nS][4] player A's behaviour thresholds
    uint16_t* mix_b;                    // [nS][4] player B's, or nullptr (uniform)
    double* alpha;                      // [2]: a step reads one slot and writes the other
    unsigned long long* steps;
    unsigned int* misuse;               // the handle's sticky words
    double gamma, decay, explor;
    int32_t nS;
    int32_t self_play;                  // mix_b follows pi_b (else it is fixed or absent)
};

// step 3 for one transition (s live, a / b in 0..4, s2 < nS)
__device__ __forceinline__ void learner_accumulate(const LearnerIO& L, uint32_t s, uint32_t a, uint32_t b, int32_t r,
                                                   uint32_t term, uint32_t s2) {
    const uint32_t cell = s * 25u + a * 5u + b;
    atomicAdd(&L.cnt[cell], 1u);
    if (r != 0) atomicAdd(&L.rsum[cell], r);
    if (!term) {
        const long long v = L.Vq[s2];
        if (v != 0ll) atomicAdd(reinterpret_cast<unsigned long long*>(&L.sv[cell]), (unsigned long long)v);
    }
}

// a behaviour policy's threshold row: SoccerBatch.mixed_policy_thresholds of (1.0 - explor) * pi + explor / 5.0
// (with explor == 0.0 this is fixed_thresholds of soccer_learners.hip operation for operation: (1.0 - 0.0) * p + 0.0 / 5.0 is p
// exactly for p >= 0, and the running sum, the floor and the clamp are the same: the populations of policy hill-climbers draw a
// FIXED player's action from its own pi row this way and get the host-computed table's bits)
__device__ __forceinline__ void learner_thresholds(const double (&pi)[5], double explor, uint16_t* row) {
    double c = 0.0;
    uint32_t t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double p = (1.0 - explor) * pi[k] + explor / 5.0;
        c = c + p;
        double f = floor(c * 32768.0 + 1e-9);
        f = f < 0.0 ? 0.0 : (f > 32768.0 ? 32768.0 : f);
        t[k] = (uint32_t)f;
    }
    *reinterpret_cast<uint2*>(row) = make_uint2(t[0] | (t[1] << 16), t[2] | (t[3] << 16));
}

// the action a 15-bit draw h takes from a threshold row: the number of thresholds <= the draw.  (pop_draw and om_pop_draw, whose
// row comes from one of two places, write the sum out: through this function their run kernels sum in another order.)
__device__ __forceinline__ uint32_t thresholds_not_above(uint2 th, uint32_t h) {
    return (h >= (th.x & 0xffffu)) + (h >= (th.x >> 16)) + (h >= (th.y & 0xffffu)) + (h >= (th.y >> 16));
}

// One lane's randomness for the step at `tick`: the environment's draw, and two action draws from one 32-bit word, 15 bits
// each (rollout_group).  (The four run kernels whose member is a thread write these lines out: through this function their
// slip-0 instantiations place two scalar instructions elsewhere, and there an instruction order has measured 1 %: DESIGN §1.)
struct StepDraws { Draw d; uint32_t ha, hb; };

template <bool SLIP>
__device__ __forceinline__ StepDraws step_draws(const KernelParams& P, unsigned long long i0, unsigned long long tick) {
    uint32_t words[1], awords[1];
    lane_words<1>(P, P.lane_offset + i0, block_tick<SLIP>(tick), 0u, words);
    lane_words<1>(P, P.lane_offset + i0, tick, 1u, awords);
    return StepDraws{draw_from_word<SLIP>(words[0], tick), awords[0] & 0x7fffu, (awords[0] >> 16) & 0x7fffu};
}

// what a state's row of everything derived from Q[s] becomes: V, Vq, the strategies, the threshold rows
__device__ __forceinline__ void learner_publish(const LearnerIO& L, int s, double v, const double (&x)[5], const double (&y)[5]) {
    L.V[s] = v;
    L.Vq[s] = (long long)rint(v * kVqScale);
#pragma unroll
    for (int k = 0; k < 5; ++k) { L.pi_a[(size_t)s * 5 + k] = x[k]; L.pi_b[(size_t)s * 5 + k] = y[k]; }
    learner_thresholds(x, L.explor, L.mix_a + (size_t)s * 4);
    if (L.self_play) learner_thresholds(y, L.explor, L.mix_b + (size_t)s * 4);
}

// ---- act, step, reduce ---------------------------------------------------------------------------
// A thread per lane, through the per-lane rule functions (lane_step) that batched_rollout's own per-lane kernel uses: the
// step costs a fraction of the three atomics behind it.
// The body both act kernels share.  NULL_A: player A's row table may be absent too (the Q-learners; minimax-Q always has
// one).  P and L by value, as a kernel takes them: by reference learner_act_kernel came out in another instruction order.
template <bool SLIP, bool LUT_LDS, bool NULL_A, class IO>
__device__ __forceinline__ void learner_act(const KernelParams P, const IO L) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    HistAcc<false> hist; hist.init(P);
    const Tables T = stage_tables<LUT_LDS>(P, smem);
    const unsigned long long tick = *P.tick_in;
    publish_tick(P, tick, 1ull);
    bool any_frozen = false;
    for (unsigned long long g = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; g < P.n;
         g += (unsigned long long)gridDim.x * kBlock) {
        const unsigned long long i0 = P.first + g;
        LaneVec<1> S; S.load(P, i0);
        const uint32_t s_now = obs_of(T, P, S.L[0].A, S.L[0].B, S.L[0].p);
        const StepDraws w = step_draws<SLIP>(P, i0, tick);
        uint32_t a, b = (w.hb * 5u) >> 15;
        if (NULL_A) a = (w.ha * 5u) >> 15;
        if (!NULL_A || L.mix_a) a = thresholds_not_above(*reinterpret_cast<const uint2*>(L.mix_a + 4u * s_now), w.ha);
        if (L.mix_b) b = thresholds_not_above(*reinterpret_cast<const uint2*>(L.mix_b + 4u * s_now), w.hb);
        StepResult R;
        const bool frozen = lane_step<SLIP, true>(T, P, S.L[0], a, b, w.d, R);
        S.store(P, i0);
        hist.add_totals(R.finished, R.reward, (uint32_t)R.reward & 1u);
        any_frozen |= frozen;
        // (a lane parked in a goal tuple by soccer_set_state has s = 0: never a current state)
        if (!frozen && s_now != 0u) learner_accumulate(L, s_now, a, b, R.reward, R.term, R.final_obs);
    }
    if (any_frozen) P.misuse[0] = 1u;
    hist.flush(P);
}

template <bool SLIP, bool LUT_LDS>
__global__ __launch_bounds__(kBlock) void learner_act_kernel(const KernelParams P, const LearnerIO L) {
    learner_act<SLIP, LUT_LDS, false>(P, L);
}

// step 3 on the caller's transitions, a thread each
template <class IO>
__device__ __forceinline__ void learner_reduce(const IO& L, long long n, const uint16_t* obs, const int8_t* act_a, const int8_t* act_b,
                                               const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs) {
    bool bad_act = false, bad_obs = false;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        const uint32_t s = obs[i], s2 = next_obs[i], a = (uint8_t)act_a[i], b = (uint8_t)act_b[i];
        const bool ba = a > 4u || b > 4u, bo = s == 0u || s >= (uint32_t)L.nS || s2 >= (uint32_t)L.nS;
        bad_act |= ba; bad_obs |= bo;
        if (!ba && !bo) learner_accumulate(L, s, a, b, (int32_t)reward[i], terminated[i] != 0u ? 1u : 0u, s2);
    }
    if (bad_act) L.misuse[1] = 1u;
    if (bad_obs) L.misuse[2] = 1u;
}

// soccer_minimax_q_update
__global__ __launch_bounds__(kBlock) void learner_reduce_kernel(const LearnerIO L, long long n, const uint16_t* obs, const int8_t* act_a,
                                                                const int8_t* act_b, const int8_t* reward, const uint8_t* terminated,
                                                                const uint16_t* next_obs) {
    learner_reduce(L, n, obs, act_a, act_b, reward, terminated, next_obs);
}

// ---- update, re-solve ----------------------------------------------------------------------------
// MODE 0: steps 4-6 of a learner step.  MODE 1 (soccer_minimax_q_load): Q is the caller's; every state with a visit is
// solved, a state without one gets what creation gives it; the accumulators, alpha and the step counter are left alone.
// MODE 2: the same with every state taken as visited.
template <int MODE>
__global__ __launch_bounds__(kLearnerBlock) void learner_update_kernel(const LearnerIO L, int slot) {
    __shared__ double sQ[kLearnerWaves][25];
    __shared__ GameWork sW[kLearnerWaves];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const int s = (int)blockIdx.x * kLearnerWaves + wave;
    const double alpha = L.alpha[slot];
    bool touched = false;
    if (s >= 1 && s < L.nS && lane < 25) {                      // index 0 is the terminal observation: Q[0] = V[0] = 0 for good
        const size_t cell = (size_t)s * 25 + lane;
        double q = L.Q[cell];
        if (MODE == 0) {
            const unsigned int c = L.cnt[cell];
            if (c != 0u) {
                const double m = ((double)L.rsum[cell] + L.gamma * ((double)L.sv[cell] * kVqInv)) / (double)c;
                q = q + alpha * (m - q);
                L.Q[cell] = q;
                L.visits[cell] += (unsigned long long)c;
                L.cnt[cell] = 0u; L.rsum[cell] = 0; L.sv[cell] = 0ll;
                touched = true;
            }
        } else {
            touched = MODE == 2 || L.visits[cell] != 0ull;
        }
        sQ[wave][lane] = q;
    }
    const bool any = __ballot(touched) != 0ull;                 // wave-uniform
    __syncthreads();
    if (s >= 1 && s < L.nS && lane == 0) {
        if (any) {
            double v = 0.0, x[5], y[5];
            solve_game5(sQ[wave], &sW[wave], &v, x, y);
            learner_publish(L, s, v, x, y);
        } else if (MODE == 1) {
            const double u[5] = {0.2, 0.2, 0.2, 0.2, 0.2};
            learner_publish(L, s, sQ[wave][0], u, u);
        }
    }
    if (MODE == 0 && blockIdx.x == 0 && threadIdx.x == 0) { L.alpha[slot ^ 1] = alpha * L.decay; *L.steps += 1ull; }
}

// creation: Q = V = q_init on the live states, uniform strategies (set, not solved), everything else zero
__global__ __launch_bounds__(kBlock) void learner_init_kernel(const LearnerIO L, double q_init, double alpha0) {
    const int cell = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (cell >= L.nS * 25) return;
    const int s = cell / 25;
    L.Q[cell] = s ? q_init : 0.0;
    L.visits[cell] = 0ull; L.cnt[cell] = 0u; L.rsum[cell] = 0; L.sv[cell] = 0ll;
    if (cell % 25 == 0) {
        const double u[5] = {0.2, 0.2, 0.2, 0.2, 0.2};
        learner_publish(L, s, s ? q_init : 0.0, u, u);
    }
    if (cell == 0) { L.alpha[0] = alpha0; L.alpha[1] = alpha0; *L.steps = 0ull; }
}

// =================================================================================================
// independent Q-learners of both players (include/soccer_hip.h, "learners, independent Q")
// =================================================================================================
// A step is the same two launches.  q_act_kernel is learner_act with the joint cell's FOUR integer accumulators (count,
// reward sum, sum of Vq_a[s'], sum of Vq_b[s']): integer sums are exact in any grouping, so the update can form a player's
// (s, own action) sums from them, and the atomics spread over 25 cells per state as minimax-Q's do.
// q_update_kernel has no stage game to solve, so a wave per state would idle: half a wave owns a state (lanes 0..24 and
// 32..56, response_sweep_kernel's layout).  Its 25 lanes bring the joint accumulators into LDS, count the visits and zero
// what they read; ten lanes (player x action) form the five sums of each player and move Q; two lanes (a player each)
// take the first maximum and write Vq and, for a GREEDY player, the threshold row of the next step.
constexpr int kQStates = 2 * kLearnerWaves;        // states per workgroup

struct QLearnerIO {
    double* Q[2];                       // [nS][5] player A's table, player B's (in B's own reward)
    long long* Vq[2];                   // [nS] rint(max_k Q_p[s][k] * 2^40)
    unsigned long long* visits;         // [nS][25]
    unsigned int* cnt;                  // [nS][25] samples of this step
    int* rsum;                          // [nS][25] sum of player A's rewards
    long long* sv[2];                   // [nS][25] sum of Vq_p[s'] over the non-terminated samples
    uint16_t* mix_a;                    // [nS][4] behaviour thresholds, or nullptr (SOCCER_QL_UNIFORM: the null row table)
    uint16_t* mix_b;
    double* alpha;                      // [2]: a step reads one slot and writes the other
    unsigned long long* steps;
    unsigned int* misuse;               // the handle's sticky words
    double gamma, decay, explor;
    int32_t nS;
    int32_t greedy[2];                  // the player's row follows its table (else it is fixed or absent)
};

__device__ __forceinline__ void learner_accumulate(const QLearnerIO& L, uint32_t s, uint32_t a, uint32_t b, int32_t r,
                                                   uint32_t term, uint32_t s2) {
    const uint32_t cell = s * 25u + a * 5u + b;
    atomicAdd(&L.cnt[cell], 1u);
    if (r != 0) atomicAdd(&L.rsum[cell], r);
    if (!term) {
        const long long va = L.Vq[0][s2], vb = L.Vq[1][s2];
        if (va != 0ll) atomicAdd(reinterpret_cast<unsigned long long*>(&L.sv[0][cell]), (unsigned long long)va);
        if (vb != 0ll) atomicAdd(reinterpret_cast<unsigned long long*>(&L.sv[1][cell]), (unsigned long long)vb);
    }
}

template <bool SLIP, bool LUT_LDS>
__global__ __launch_bounds__(kBlock) void q_act_kernel(const KernelParams P, const QLearnerIO L) {
    learner_act<SLIP, LUT_LDS, true>(P, L);
}

// soccer_q_learner_update
__global__ __launch_bounds__(kBlock) void q_reduce_kernel(const QLearnerIO L, long long n, const uint16_t* obs, const int8_t* act_a,
                                                          const int8_t* act_b, const int8_t* reward, const uint8_t* terminated,
                                                          const uint16_t* next_obs) {
    learner_reduce(L, n, obs, act_a, act_b, reward, terminated, next_obs);
}

// MODE 0: steps 4-6 of a learner step.  MODE 1 (creation, soccer_q_learner_load): every row derived from Q is recomputed,
// row 0 included; the accumulators, the counts, alpha and the step counter are left alone.
template <int MODE>
__global__ __launch_bounds__(kLearnerBlock) void q_update_kernel(const QLearnerIO L, int slot) {
    __shared__ unsigned int sC[kQStates][25];
    __shared__ int sR[kQStates][25];
    __shared__ long long sS[2][kQStates][25];
    __shared__ double sQ[kQStates][10];
    const int st = (int)(threadIdx.x >> 5), lane = (int)(threadIdx.x & 31u);
    const int s = (int)blockIdx.x * kQStates + st;
    const bool live = s < L.nS && (MODE == 1 || s >= 1);        // index 0 is the terminal observation: Q_p[0] = 0 for good
    const double alpha = L.alpha[slot];
    unsigned int c = 0u;
    if (MODE == 0 && live && lane < 25) {
        // both players' sums are read here, before anything is zeroed
        const size_t cell = (size_t)s * 25 + lane;
        c = L.cnt[cell];
        sC[st][lane] = c;
        if (c != 0u) {
            sR[st][lane] = L.rsum[cell]; sS[0][st][lane] = L.sv[0][cell]; sS[1][st][lane] = L.sv[1][cell];
            L.visits[cell] += (unsigned long long)c;
            L.cnt[cell] = 0u; L.rsum[cell] = 0; L.sv[0][cell] = 0ll; L.sv[1][cell] = 0ll;
        } else {
            sR[st][lane] = 0; sS[0][st][lane] = 0ll; sS[1][st][lane] = 0ll;
        }
    }
    // the half-wave's 25 bits of the wave's ballot: was any cell of this state touched?
    const bool any = MODE == 1 || (((unsigned long long)__ballot(c != 0u) >> (threadIdx.x & 32u)) & 0x1ffffffull) != 0ull;
    __syncthreads();
    if (live && lane < 10) {
        const int p = lane / 5, k = lane - 5 * p;                // player, own action
        const size_t row = (size_t)s * 5 + k;
        double q = L.Q[p][row];
        if (MODE == 0) {
            unsigned int cc = 0u; long long R = 0ll, SV = 0ll;
#pragma unroll
            for (int j = 0; j < 5; ++j) {                        // over the other player's action
                const int x = p ? j * 5 + k : k * 5 + j;
                cc += sC[st][x]; R += (long long)sR[st][x]; SV += sS[p][st][x];
            }
            if (cc != 0u) {
                if (p) R = -R;                                   // player B's own reward
                const double m = ((double)R + L.gamma * ((double)SV * kVqInv)) / (double)cc;
                q = q + alpha * (m - q);
                L.Q[p][row] = q;
            }
        }
        sQ[st][lane] = q;
    }
    __syncthreads();
    if (live && any && lane < 2) {
        const int p = lane;
        double v = sQ[st][p * 5];
        int g = 0;
#pragma unroll
        for (int k = 1; k < 5; ++k) {
            const double r = sQ[st][p * 5 + k];
            if (r > v) { v = r; g = k; }                         // the first index that attains it
        }
        L.Vq[p][s] = (long long)rint(v * kVqScale);
        if (L.greedy[p]) {
            double pi[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) pi[k] = k == g ? 1.0 : 0.0;
            learner_thresholds(pi, L.explor, (p ? L.mix_b : L.mix_a) + (size_t)s * 4);
        }
    }
    if (MODE == 0 && blockIdx.x == 0 && threadIdx.x == 0) { L.alpha[slot ^ 1] = alpha * L.decay; *L.steps += 1ull; }
}

// creation: Q_p = q_init on the live states, everything else zero (q_update_kernel<1> then derives the rows)
__global__ __launch_bounds__(kBlock) void q_init_kernel(const QLearnerIO L, double q_init, double alpha0) {
    const int cell = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (cell >= L.nS * 25) return;
    const int s = cell / 25, k = cell % 25;
    if (k < 10) L.Q[k / 5][(size_t)s * 5 + k % 5] = s ? q_init : 0.0;
    L.visits[cell] = 0ull; L.cnt[cell] = 0u; L.rsum[cell] = 0; L.sv[0][cell] = 0ll; L.sv[1][cell] = 0ll;
    if (cell == 0) { L.alpha[0] = alpha0; L.alpha[1] = alpha0; *L.steps = 0ull; }
}

// =================================================================================================
// policy hill-climbing learners of both players (include/soccer_hip.h, "learners, policy hill-climbing")
// =================================================================================================
// The Q-learners with an explicit mixed policy per player.  PhcIO begins with a QLearnerIO, so the act body, the reduce body
// and learner_accumulate are the Q-learners' own (greedy[] is not used: a LEARN player's row follows pi, not the table).
// phc_update_kernel is q_update_kernel up to the two lanes that own a player: after the first maximum and Vq they run the
// policy step (step 5) for a LEARN player and write pi, avg and the threshold row of the next step.  Everything there is
// unrolled over k with the greedy index compared, never used as a subscript: the rows stay in registers.
struct PhcIO : QLearnerIO {
    double* pi[2];                      // [nS][5] the policies
    double* avg[2];                     // [nS][5] their running averages
    unsigned long long* updates;        // [nS] learner steps that touched the state
    double* dscale;                     // [2]: two slots, as alpha
    double delta_win, delta_lose, delta_decay;
    int32_t learn[2];                   // the player's pi, avg and row are updated (else they are constant)
};

template <bool SLIP, bool LUT_LDS>
__global__ __launch_bounds__(kBlock) void phc_act_kernel(const KernelParams P, const PhcIO L) {
    learner_act<SLIP, LUT_LDS, true>(P, L);
}

// soccer_wolf_phc_update
__global__ __launch_bounds__(kBlock) void phc_reduce_kernel(const PhcIO L, long long n, const uint16_t* obs, const int8_t* act_a,
                                                            const int8_t* act_b, const int8_t* reward, const uint8_t* terminated,
                                                            const uint16_t* next_obs) {
    learner_reduce(L, n, obs, act_a, act_b, reward, terminated, next_obs);
}

// MODE 0: steps 4-6 of a learner step.  MODE 1 (creation, soccer_wolf_phc_load): Vq and the LEARN players' threshold rows are
// recomputed from Q and pi, row 0 included; everything else is left alone.
template <int MODE>
__global__ __launch_bounds__(kLearnerBlock) void phc_update_kernel(const PhcIO L, int slot) {
    __shared__ unsigned int sC[kQStates][25];
    __shared__ int sR[kQStates][25];
    __shared__ long long sS[2][kQStates][25];
    __shared__ double sQ[kQStates][10];
    __shared__ unsigned long long sN[kQStates];
    const int st = (int)(threadIdx.x >> 5), lane = (int)(threadIdx.x & 31u);
    const int s = (int)blockIdx.x * kQStates + st;
    const bool live = s < L.nS && (MODE == 1 || s >= 1);        // index 0 is the terminal observation: Q_p[0] = 0 for good
    const double alpha = L.alpha[slot], dscale = L.dscale[slot];
    unsigned int c = 0u;
    if (MODE == 0 && live && lane < 25) {
        // both players' sums are read here, before anything is zeroed
        const size_t cell = (size_t)s * 25 + lane;
        c = L.cnt[cell];
        sC[st][lane] = c;
        if (c != 0u) {
            sR[st][lane] = L.rsum[cell]; sS[0][st][lane] = L.sv[0][cell]; sS[1][st][lane] = L.sv[1][cell];
            L.visits[cell] += (unsigned long long)c;
            L.cnt[cell] = 0u; L.rsum[cell] = 0; L.sv[0][cell] = 0ll; L.sv[1][cell] = 0ll;
        } else {
            sR[st][lane] = 0; sS[0][st][lane] = 0ll; sS[1][st][lane] = 0ll;
        }
    }
    // the half-wave's 25 bits of the wave's ballot: was any cell of this state touched?
    const bool any = MODE == 1 || (((unsigned long long)__ballot(c != 0u) >> (threadIdx.x & 32u)) & 0x1ffffffull) != 0ull;
    __syncthreads();
    if (live && lane < 10) {
        const int p = lane / 5, k = lane - 5 * p;                // player, own action
        const size_t row = (size_t)s * 5 + k;
        double q = L.Q[p][row];
        if (MODE == 0) {
            unsigned int cc = 0u; long long R = 0ll, SV = 0ll;
#pragma unroll
            for (int j = 0; j < 5; ++j) {                        // over the other player's action
                const int x = p ? j * 5 + k : k * 5 + j;
                cc += sC[st][x]; R += (long long)sR[st][x]; SV += sS[p][st][x];
            }
            if (cc != 0u) {
                if (p) R = -R;                                   // player B's own reward
                const double m = ((double)R + L.gamma * ((double)SV * kVqInv)) / (double)cc;
                q = q + alpha * (m - q);
                L.Q[p][row] = q;
            }
            if (lane == 0 && any) {                              // both player lanes need the count: through LDS, one writer
                const unsigned long long n = L.updates[s] + 1ull;
                L.updates[s] = n;
                sN[st] = n;
            }
        }
        sQ[st][lane] = q;
    }
    __syncthreads();
    if (live && any && lane < 2) {
        const int p = lane;
        double Q[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) Q[k] = sQ[st][p * 5 + k];
        double v = Q[0];
        int g = 0;
#pragma unroll
        for (int k = 1; k < 5; ++k)
            if (Q[k] > v) { v = Q[k]; g = k; }                   // the first index that attains it
        L.Vq[p][s] = (long long)rint(v * kVqScale);
        if (L.learn[p]) {
            double* const gpi = L.pi[p] + (size_t)s * 5;
            double pi[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) pi[k] = gpi[k];
            if (MODE == 0) {                                     // step 5
                double* const gavg = L.avg[p] + (size_t)s * 5;
                const double n = (double)sN[st];
                double avg[5], ep = 0.0, ea = 0.0;
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    avg[k] = gavg[k];
                    avg[k] = avg[k] + (pi[k] - avg[k]) / n;
                }
#pragma unroll
                for (int k = 0; k < 5; ++k) { ep = ep + pi[k] * Q[k]; ea = ea + avg[k] * Q[k]; }
                const double d = ((ep > ea ? L.delta_win : L.delta_lose) * dscale) / 4.0;
                double moved = 0.0;
#pragma unroll
                for (int k = 0; k < 5; ++k)
                    if (k != g) {
                        const double m = pi[k] < d ? pi[k] : d;
                        pi[k] = pi[k] - m;
                        moved = moved + m;
                    }
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    if (k == g) pi[k] = pi[k] + moved;
                    gpi[k] = pi[k]; gavg[k] = avg[k];
                }
            }
            learner_thresholds(pi, L.explor, (p ? L.mix_b : L.mix_a) + (size_t)s * 4);
        }
    }
    if (MODE == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
        L.alpha[slot ^ 1] = alpha * L.decay; L.dscale[slot ^ 1] = dscale * L.delta_decay; *L.steps += 1ull;
    }
}

// creation: Q_p = q_init on the live states, 0.2 rows (a FIXED player's are copied over them), dscale = 1, everything else
// zero (phc_update_kernel<1> then derives the rows)
__global__ __launch_bounds__(kBlock) void phc_init_kernel(const PhcIO L, double q_init, double alpha0) {
    const int cell = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (cell >= L.nS * 25) return;
    const int s = cell / 25, k = cell % 25;
    if (k < 10) {
        const size_t row = (size_t)s * 5 + k % 5;
        L.Q[k / 5][row] = s ? q_init : 0.0;
        L.pi[k / 5][row] = 0.2; L.avg[k / 5][row] = 0.2;
    }
    if (k == 0) L.updates[s] = 0ull;
    L.visits[cell] = 0ull; L.cnt[cell] = 0u; L.rsum[cell] = 0; L.sv[0][cell] = 0ll; L.sv[1][cell] = 0ll;
    if (cell == 0) { L.alpha[0] = alpha0; L.alpha[1] = alpha0; L.dscale[0] = 1.0; L.dscale[1] = 1.0; *L.steps = 0ull; }
}

// =================================================================================================
// regret matchers of both players, one table (include/soccer_hip.h, "learners, regret matching")
// =================================================================================================
// The hill-climbers with the policy derived from cumulative regrets instead of stored.  RmIO begins with a QLearnerIO, so the
// act body, the reduce body and learner_accumulate are the Q-learners' own (greedy[] is not used); Vq_p is the value of the
// player's own policy, not the row maximum, and only rm_update_kernel knows.  rm_update_kernel is phc_update_kernel up to the
// two lanes that own a player: they run step 5 and write R, Z, Vq_p and a LEARN player's threshold row of the next step.  A
// state has one owner and R is read before it is written, so "the policy from R as it was before this step" needs no copy.
// Everything there is unrolled over k: the rows stay in registers.
struct RmIO : QLearnerIO {
    double* R[2];                       // [nS][5] the cumulative regrets
    double* Z[2];                       // [nS][5] the policy sums
    unsigned long long* updates;        // [nS] learner steps that touched the state
    const double* fixed[2];             // [nS][5] a FIXED player's rows (its Vq needs them); else nullptr
    int32_t learn[2];                   // the player's R, Z and row are updated; else it is FIXED (fixed[p]) or UNIFORM (0.2 rows)
    int32_t plus, linear;               // regrets floored at 0; a step's policy weighed by the state's update count
};

// policy(p, s) of the header for a LEARN player from its five regrets: rm_policy (of the population, below) on a row of five
__device__ __forceinline__ void rm_policy5(const double (&R)[5], double (&pi)[5]) {
    double pos[5], tot = 0.0;
#pragma unroll
    for (int k = 0; k < 5; ++k) { pos[k] = R[k] > 0.0 ? R[k] : 0.0; tot = tot + pos[k]; }
#pragma unroll
    for (int k = 0; k < 5; ++k) pi[k] = tot > 0.0 ? pos[k] / tot : 0.2;
}

template <bool SLIP, bool LUT_LDS>
__global__ __launch_bounds__(kBlock) void rm_act_kernel(const KernelParams P, const RmIO L) {
    learner_act<SLIP, LUT_LDS, true>(P, L);
}

// soccer_regret_learner_update
__global__ __launch_bounds__(kBlock) void rm_reduce_kernel(const RmIO L, long long n, const uint16_t* obs, const int8_t* act_a,
                                                           const int8_t* act_b, const int8_t* reward, const uint8_t* terminated,
                                                           const uint16_t* next_obs) {
    learner_reduce(L, n, obs, act_a, act_b, reward, terminated, next_obs);
}

// MODE 0: steps 4-6 of a learner step.  MODE 1 (creation, soccer_regret_learner_load): Vq and the LEARN players' threshold
// rows are recomputed from Q and R, row 0 included; everything else is left alone.
template <int MODE>
__global__ __launch_bounds__(kLearnerBlock) void rm_update_kernel(const RmIO L, int slot) {
    __shared__ unsigned int sC[kQStates][25];
    __shared__ int sR[kQStates][25];
    __shared__ long long sS[2][kQStates][25];
    __shared__ double sQ[kQStates][10];
    __shared__ unsigned long long sN[kQStates];
    const int st = (int)(threadIdx.x >> 5), lane = (int)(threadIdx.x & 31u);
    const int s = (int)blockIdx.x * kQStates + st;
    const bool live = s < L.nS && (MODE == 1 || s >= 1);        // index 0 is the terminal observation: Q_p[0] = 0 for good
    const double alpha = L.alpha[slot];
    unsigned int c = 0u;
    if (MODE == 0 && live && lane < 25) {
        // both players' sums are read here, before anything is zeroed
        const size_t cell = (size_t)s * 25 + lane;
        c = L.cnt[cell];
        sC[st][lane] = c;
        if (c != 0u) {
            sR[st][lane] = L.rsum[cell]; sS[0][st][lane] = L.sv[0][cell]; sS[1][st][lane] = L.sv[1][cell];
            L.visits[cell] += (unsigned long long)c;
            L.cnt[cell] = 0u; L.rsum[cell] = 0; L.sv[0][cell] = 0ll; L.sv[1][cell] = 0ll;
        } else {
            sR[st][lane] = 0; sS[0][st][lane] = 0ll; sS[1][st][lane] = 0ll;
        }
    }
    // the half-wave's 25 bits of the wave's ballot: was any cell of this state touched?
    const bool any = MODE == 1 || (((unsigned long long)__ballot(c != 0u) >> (threadIdx.x & 32u)) & 0x1ffffffull) != 0ull;
    __syncthreads();
    if (live && lane < 10) {
        const int p = lane / 5, k = lane - 5 * p;                // player, own action
        const size_t row = (size_t)s * 5 + k;
        double q = L.Q[p][row];
        if (MODE == 0) {
            unsigned int cc = 0u; long long R = 0ll, SV = 0ll;
#pragma unroll
            for (int j = 0; j < 5; ++j) {                        // over the other player's action
                const int x = p ? j * 5 + k : k * 5 + j;
                cc += sC[st][x]; R += (long long)sR[st][x]; SV += sS[p][st][x];
            }
            if (cc != 0u) {
                if (p) R = -R;                                   // player B's own reward
                const double m = ((double)R + L.gamma * ((double)SV * kVqInv)) / (double)cc;
                q = q + alpha * (m - q);
                L.Q[p][row] = q;
            }
            if (lane == 0 && any) {                              // both player lanes need the count: through LDS, one writer
                const unsigned long long n = L.updates[s] + 1ull;
                L.updates[s] = n;
                sN[st] = n;
            }
        }
        sQ[st][lane] = q;
    }
    __syncthreads();
    if (live && any && lane < 2) {
        const int p = lane;
        double Q[5], pi[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) Q[k] = sQ[st][p * 5 + k];
        if (L.learn[p]) {
            double* const gR = L.R[p] + (size_t)s * 5;
            double R[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) R[k] = gR[k];
            rm_policy5(R, pi);                                   // from R as it was before this step
            if (MODE == 0) {                                     // step 5
                double* const gZ = L.Z[p] + (size_t)s * 5;
                const double w = L.linear ? (double)sN[st] : 1.0;
                double u = 0.0;
#pragma unroll
                for (int k = 0; k < 5; ++k) u = u + pi[k] * Q[k];
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    double x = R[k] + (Q[k] - u);
                    if (L.plus) x = x > 0.0 ? x : 0.0;
                    R[k] = x;
                    gR[k] = x;
                    gZ[k] = gZ[k] + w * pi[k];
                }
                rm_policy5(R, pi);                               // the policy the next step acts from
            }
            learner_thresholds(pi, L.explor, (p ? L.mix_b : L.mix_a) + (size_t)s * 4);
        } else if (L.fixed[p]) {
            const double* const row = L.fixed[p] + (size_t)s * 5;
#pragma unroll
            for (int k = 0; k < 5; ++k) pi[k] = row[k];
        } else {
#pragma unroll
            for (int k = 0; k < 5; ++k) pi[k] = 0.2;
        }
        double v = 0.0;                                          // the value of the player's own policy stands where the maximum stood
#pragma unroll
        for (int k = 0; k < 5; ++k) v = v + pi[k] * Q[k];
        L.Vq[p][s] = (long long)rint(v * kVqScale);
    }
    if (MODE == 0 && blockIdx.x == 0 && threadIdx.x == 0) { L.alpha[slot ^ 1] = alpha * L.decay; *L.steps += 1ull; }
}

// creation: Q_p = q_init on the live states, R = Z = 0, everything else zero (rm_update_kernel<1> then derives the rows)
__global__ __launch_bounds__(kBlock) void rm_init_kernel(const RmIO L, double q_init, double alpha0) {
    const int cell = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (cell >= L.nS * 25) return;
    const int s = cell / 25, k = cell % 25;
    if (k < 10) {
        const size_t row = (size_t)s * 5 + k % 5;
        L.Q[k / 5][row] = s ? q_init : 0.0;
        L.R[k / 5][row] = 0.0; L.Z[k / 5][row] = 0.0;
    }
    if (k == 0) L.updates[s] = 0ull;
    L.visits[cell] = 0ull; L.cnt[cell] = 0u; L.rsum[cell] = 0; L.sv[0][cell] = 0ll; L.sv[1][cell] = 0ll;
    if (cell == 0) { L.alpha[0] = alpha0; L.alpha[1] = alpha0; *L.steps = 0ull; }
}

// =================================================================================================
// a population of independent Q-learners, a learner per lane (include/soccer_hip.h, "learners, a population ...")
// =================================================================================================
// Member i is a Q-learner whose only actor is lane i, so nothing is shared between threads: no accumulators, no atomics, no
// second launch.  pop_run_kernel is rollout_kernel's per-lane loop (state in registers over the launch's steps) with the
// update inside it; a thread owns lane i and member i's tables.
// Table layout: member i's block is [nS][2][5] float64 — the row of player A and the row of player B of one state are the
// 80 adjacent, 16-byte aligned bytes a step needs together (five 16-byte loads, one or two cache lines), and a member's
// block is contiguous, so a range of members is one copy.
// Per step the dependent chain is ONE row gather, at s' for the bootstrap: the row at s (for the greedy draw and the
// update) is carried in registers — it is the previous step's s' row while the episode goes on, patched when the update
// wrote into that very row (s' == s: every blocked move, every STAND), and loaded only after a reset.  The two moved
// entries are stored straight away, so memory always holds what the registers do.
// Everything is unrolled over the five actions with the action / greedy index COMPARED, never used as a subscript: the rows
// stay in registers (0 bytes of scratch).
struct PopIO {
    double* Q;                          // [n][nS][2][5]
    double* alpha;                      // [n] every member's learning rate
    const double* decay;                // [n]
    const double* explor;               // [n]
    const double* gamma;                // [n]
    const uint16_t* mix[2];             // [nS][4] a FIXED player's thresholds, shared by all members; else nullptr
    unsigned long long* steps;
    unsigned int* misuse;               // the handle's sticky words
    int32_t nS;
    int32_t n_steps;                    // pop_run_kernel: steps of this launch
    int32_t mode[2];                    // SOCCER_QL_* of player A, player B
};
constexpr int kPopGreedy = 0, kPopUniform = 1;      // = SOCCER_QL_GREEDY, SOCCER_QL_UNIFORM (soccer_learners.hip asserts it)

__device__ __forceinline__ void pop_load_row(const double* tab, uint32_t s, double (&row)[10]) {
    const double2* p = reinterpret_cast<const double2*>(tab + (size_t)s * 10);
#pragma unroll
    for (int k = 0; k < 5; ++k) { const double2 v = p[k]; row[2 * k] = v.x; row[2 * k + 1] = v.y; }
}

// steps 3-5 of one member on its one transition: `row` = its rows at s (A's five, B's five), `nxt` = its rows at s' as they
// were BEFORE this update.  c = 1, so the mean target is the sample's own: m = R + gamma * SV * 2^-40 on the learners' grid.
// Moves row[a] and row[5 + b] and hands the two new values back for the store.
__device__ __forceinline__ void pop_learn(double (&row)[10], const double (&nxt)[10], uint32_t a, uint32_t b, int32_t r,
                                          uint32_t term, double alpha, double gamma, double& qa, double& qb) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        double v = nxt[5 * p];
#pragma unroll
        for (int k = 1; k < 5; ++k) v = nxt[5 * p + k] > v ? nxt[5 * p + k] : v;
        const long long SV = term ? 0ll : (long long)rint(v * kVqScale);
        const long long R = p ? -(long long)r : (long long)r;                   // player B's own reward
        const double m = (double)R + gamma * ((double)SV * kVqInv);
        const uint32_t act = p ? b : a;
        double q = 0.0;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const double old = row[5 * p + k];
            const double moved = old + alpha * (m - old);
            row[5 * p + k] = (uint32_t)k == act ? moved : old;
            q = (uint32_t)k == act ? moved : q;
        }
        (p ? qb : qa) = q;
    }
}

// a player's action from its 15-bit draw h: the null row table, the shared fixed rows, or epsilon-greedy on its own row
__device__ __forceinline__ uint32_t pop_draw(const PopIO& L, int p, const double (&row)[10], uint32_t s, double explor, uint32_t h) {
    if (L.mode[p] == kPopUniform) return (h * 5u) >> 15;                       // wave-uniform
    uint2 th;
    if (L.mode[p] == kPopGreedy) {
        double v = row[5 * p];
        int g = 0;
#pragma unroll
        for (int k = 1; k < 5; ++k)
            if (row[5 * p + k] > v) { v = row[5 * p + k]; g = k; }              // the first index that attains it
        double pi[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) pi[k] = k == g ? 1.0 : 0.0;
        __attribute__((aligned(8))) uint16_t t[4];
        learner_thresholds(pi, explor, t);
        th = *reinterpret_cast<const uint2*>(t);
    } else {
        th = *reinterpret_cast<const uint2*>(L.mix[p] + 4u * s);
    }
    return (h >= (th.x & 0xffffu)) + (h >= (th.x >> 16)) + (h >= (th.y & 0xffffu)) + (h >= (th.y >> 16));
}

template <bool SLIP, bool LUT_LDS>
__global__ __launch_bounds__(kBlock) void pop_run_kernel(const KernelParams P, const PopIO L) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    HistAcc<false> hist; hist.init(P);
    const Tables T = stage_tables<LUT_LDS>(P, smem);
    const unsigned long long tick0 = *P.tick_in;
    publish_tick(P, tick0, (unsigned long long)L.n_steps);
    if (blockIdx.x == 0 && threadIdx.x == 0) *L.steps += (unsigned long long)L.n_steps;
    bool any_frozen = false;
    for (unsigned long long g = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; g < P.n;
         g += (unsigned long long)gridDim.x * kBlock) {
        const unsigned long long i0 = P.first + g;                  // the lane, and the member
        LaneVec<1> S; S.load(P, i0);
        double* const tab = L.Q + (size_t)i0 * (size_t)L.nS * 10;
        double alpha = L.alpha[i0];
        const double decay = L.decay[i0], explor = L.explor[i0], gamma = L.gamma[i0];
        uint32_t s = obs_of(T, P, S.L[0].A, S.L[0].B, S.L[0].p);
        double row[10];
        pop_load_row(tab, s, row);
        int32_t ret = 0; uint32_t eps = 0u, nonzero = 0u;
        for (int t = 0; t < L.n_steps; ++t) {
            const unsigned long long tick = tick0 + (unsigned long long)t;
            uint32_t words[1], awords[1];
            lane_words<1>(P, P.lane_offset + i0, block_tick<SLIP>(tick), 0u, words);
            lane_words<1>(P, P.lane_offset + i0, tick, 1u, awords);
            const Draw d = draw_from_word<SLIP>(words[0], tick);
            // two actions from one 32-bit word, 15 bits each (rollout_group)
            const uint32_t a = pop_draw(L, 0, row, s, explor, awords[0] & 0x7fffu);
            const uint32_t b = pop_draw(L, 1, row, s, explor, (awords[0] >> 16) & 0x7fffu);
            StepResult R;
            const bool frozen = lane_step<SLIP, true>(T, P, S.L[0], a, b, d, R);
            ret += R.reward; eps += R.finished; nonzero += (uint32_t)R.reward & 1u;
            any_frozen |= frozen;
            // (a lane parked in a goal tuple by soccer_set_state has s = 0: never a current state)
            const bool learn = !frozen && s != 0u;
            const uint32_t s2 = R.final_obs, sn = R.obs;
            double nxt[10];
            if (learn) {
                pop_load_row(tab, s2, nxt);                         // before the stores below: s' may be s
                double qa, qb;
                pop_learn(row, nxt, a, b, R.reward, R.term, alpha, gamma, qa, qb);
                double* const at = tab + (size_t)s * 10;
                at[a] = qa; at[5u + b] = qb;
            }
            if (learn && sn == s2) {                                // the episode goes on: the row at s' is the next row at s
                if (s2 != s) {
#pragma unroll
                    for (int k = 0; k < 10; ++k) row[k] = nxt[k];
                }                                                   // (s' == s: `row` already holds what the update wrote)
            } else if (sn != s) {
                pop_load_row(tab, sn, row);                         // after a reset
            }
            s = sn;
            alpha = alpha * decay;
        }
        S.store(P, i0);
        L.alpha[i0] = alpha;
        hist.add_totals(eps, ret, nonzero);
    }
    if (any_frozen) P.misuse[0] = 1u;
    hist.flush(P);
}

// ---- a league opponent (include/soccer_hip.h, "learners, a league opponent for the population of Q-learners") ----------
// pop_run_kernel with one word more per member: `pick`, the league policy its lane's league player follows until the
// episode ends.  pick lives in a register over the launch (loaded once, stored once, like alpha).  The league player's
// threshold row is one 8-byte load at (pick, s) from the [K][nS][4] table; the other player draws through pop_draw as in
// pop_run_kernel.  A pick is drawn only under pick < 0 — the Philox block of purpose 1 at counter 2^62 + tick and the
// bisection of the cumulative table T (soccer_league.hpp) sit inside that branch.  T stays in global memory: a lane probes
// it at its own index (a vector load, not a scalar one), at most ten dependent loads of an 8 KB table that lives in L2
// once per EPISODE of a lane, against one row gather per STEP; staging it in LDS would cost every workgroup K - 1 loads
// and a barrier per launch to save those.  Unmeasured.
struct PopLeagueIO {
    const uint16_t* thr;                // [K][nS][4] the league policies' thresholds
    const uint64_t* T;                  // [K - 1] the weights' cumulative thresholds, never decreasing, <= 2^32
    int32_t* pick;                      // [n] -1: draw at the next step
    int32_t K;
    int32_t player;                     // 0: player A is the league, 1: player B
};

__device__ __forceinline__ uint32_t league_draw(const PopLeagueIO& G, int32_t nS, int32_t pick, uint32_t s, uint32_t h) {
    // (K * nS * 4 <= 2^10 * 2^16 * 4: the index fits 32 bits)
    return thresholds_not_above(*reinterpret_cast<const uint2*>(G.thr + 4u * ((uint32_t)pick * (uint32_t)nS + s)), h);
}

template <bool SLIP, bool LUT_LDS>
__global__ __launch_bounds__(kBlock) void pop_league_run_kernel(const KernelParams P, const PopIO L, const PopLeagueIO G) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    HistAcc<false> hist; hist.init(P);
    const Tables T = stage_tables<LUT_LDS>(P, smem);
    const unsigned long long tick0 = *P.tick_in;
    publish_tick(P, tick0, (unsigned long long)L.n_steps);
    if (blockIdx.x == 0 && threadIdx.x == 0) *L.steps += (unsigned long long)L.n_steps;
    bool any_frozen = false;
    for (unsigned long long g = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; g < P.n;
         g += (unsigned long long)gridDim.x * kBlock) {
        const unsigned long long i0 = P.first + g;                  // the lane, and the member
        LaneVec<1> S; S.load(P, i0);
        double* const tab = L.Q + (size_t)i0 * (size_t)L.nS * 10;
        double alpha = L.alpha[i0];
        const double decay = L.decay[i0], explor = L.explor[i0], gamma = L.gamma[i0];
        int32_t pick = G.pick[i0];
        uint32_t s = obs_of(T, P, S.L[0].A, S.L[0].B, S.L[0].p);
        double row[10];
        pop_load_row(tab, s, row);
        int32_t ret = 0; uint32_t eps = 0u, nonzero = 0u;
        for (int t = 0; t < L.n_steps; ++t) {
            const unsigned long long tick = tick0 + (unsigned long long)t;
            uint32_t words[1], awords[1];
            lane_words<1>(P, P.lane_offset + i0, block_tick<SLIP>(tick), 0u, words);
            lane_words<1>(P, P.lane_offset + i0, tick, 1u, awords);
            const Draw d = draw_from_word<SLIP>(words[0], tick);
            if (__builtin_expect(pick < 0, 0)) {                                         // kick-off: frozen and parked lanes draw too
                uint32_t lw[1];
                lane_words<1>(P, P.lane_offset + i0, (1ull << 62) + tick, 1u, lw);
                pick = league_pick(G.T, G.K - 1, lw[0]);
            }
            const uint32_t ha = awords[0] & 0x7fffu, hb = (awords[0] >> 16) & 0x7fffu;
            // (one branch on the league's player, not a select per action: with selects the slip-0 instantiations kept a
            // dead 68-byte frame — a scalar tuple the allocator planned to spill and then reloaded from the kernel arguments)
            uint32_t a, b;
            if (G.player == 0) { a = league_draw(G, L.nS, pick, s, ha); b = pop_draw(L, 1, row, s, explor, hb); }   // (wave-uniform)
            else { a = pop_draw(L, 0, row, s, explor, ha); b = league_draw(G, L.nS, pick, s, hb); }
            StepResult R;
            const bool frozen = lane_step<SLIP, true>(T, P, S.L[0], a, b, d, R);
            ret += R.reward; eps += R.finished; nonzero += (uint32_t)R.reward & 1u;
            any_frozen |= frozen;
            pick = R.finished ? -1 : pick;                          // the next episode draws again
            const bool learn = !frozen && s != 0u;
            const uint32_t s2 = R.final_obs, sn = R.obs;
            double nxt[10];
            if (learn) {
                pop_load_row(tab, s2, nxt);                         // before the stores below: s' may be s
                double qa, qb;
                pop_learn(row, nxt, a, b, R.reward, R.term, alpha, gamma, qa, qb);
                double* const at = tab + (size_t)s * 10;
                at[a] = qa; at[5u + b] = qb;
            }
            if (learn && sn == s2) {                                // the episode goes on: the row at s' is the next row at s
                if (s2 != s) {
#pragma unroll
                    for (int k = 0; k < 10; ++k) row[k] = nxt[k];
                }
            } else if (sn != s) {
                pop_load_row(tab, sn, row);                         // after a reset
            }
            s = sn;
            alpha = alpha * decay;
        }
        S.store(P, i0);
        L.alpha[i0] = alpha;
        G.pick[i0] = pick;
        hist.add_totals(eps, ret, nonzero);
    }
    if (any_frozen) P.misuse[0] = 1u;
    hist.flush(P);
}

// soccer_q_population_update: steps 3-6 on the caller's transitions, transition i for member i
__global__ __launch_bounds__(kBlock) void pop_update_kernel(const PopIO L, long long n, const uint16_t* obs, const int8_t* act_a,
                                                            const int8_t* act_b, const int8_t* reward, const uint8_t* terminated,
                                                            const uint16_t* next_obs) {
    bool bad_act = false, bad_obs = false;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        const uint32_t s = obs[i], s2 = next_obs[i], a = (uint8_t)act_a[i], b = (uint8_t)act_b[i];
        const bool ba = a > 4u || b > 4u, bo = s == 0u || s >= (uint32_t)L.nS || s2 >= (uint32_t)L.nS;
        bad_act |= ba; bad_obs |= bo;
        const double alpha = L.alpha[i];
        if (!ba && !bo) {
            double* const tab = L.Q + (size_t)i * (size_t)L.nS * 10;
            double row[10], nxt[10], qa, qb;
            pop_load_row(tab, s, row);
            pop_load_row(tab, s2, nxt);
            pop_learn(row, nxt, a, b, (int32_t)reward[i], terminated[i] != 0u ? 1u : 0u, alpha, L.gamma[i], qa, qb);
            double* const at = tab + (size_t)s * 10;
            at[a] = qa; at[5u + b] = qb;
        }
        L.alpha[i] = alpha * L.decay[i];
    }
    if (bad_act) L.misuse[1] = 1u;
    if (bad_obs) L.misuse[2] = 1u;
    if (blockIdx.x == 0 && threadIdx.x == 0) *L.steps += 1ull;
}

// creation: every member's Q_p = q_init on the live states, row 0 zero
__global__ __launch_bounds__(kBlock) void pop_init_kernel(const PopIO L, unsigned long long n, double q_init) {
    const unsigned long long per = (unsigned long long)L.nS * 10ull, cells = n * per;
    for (unsigned long long c = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; c < cells; c += (unsigned long long)gridDim.x * kBlock)
        L.Q[c] = (c % per) < 10ull ? 0.0 : q_init;
    if (blockIdx.x == 0 && threadIdx.x == 0) *L.steps = 0ull;
}

// =================================================================================================
// a population of policy hill-climbers, a learner per lane (include/soccer_hip.h, "learners, a population of policy hill-climbers")
// =================================================================================================
// Member i is a soccer_wolf_phc learner whose only actor is lane i: pop_run_kernel's shape (a thread owns lane i and member i,
// the lane and the rows of the current state in registers over the launch's steps, no atomics, no second launch) with the
// policy step behind the Q update.  lane_words / draw_from_word / lane_step / learner_thresholds / pop_learn are the same
// functions the other learners call.
// Table layout: member i's block is [nS][32] float64, one 256-byte aligned row per state:
//     0..4 Q_a   5..9 Q_b   10..14 pi_a   15..19 avg_a   20..24 pi_b   25..29 avg_b   30 updates (uint64)   31 pad
// so everything a step needs at s is two cache lines, Q_a | Q_b and pi_p | avg_p are runs of ten values on a 16-byte
// boundary, and a member's block is contiguous.
// What a step carries: Q_a, Q_b, pi_a, pi_b at s (the next draw and, as the previous step's s' rows, the bootstrap), as
// pop_run_kernel carries Q.  avg and updates at s are used only after the environment step: their loads are issued at the
// top of the step and nothing of them lives across steps.  Everything is unrolled over the five actions with the action /
// greedy index COMPARED, never used as a subscript: the rows stay in registers (0 bytes of scratch).
constexpr int kPhcRow = 32;                         // float64 slots per state
constexpr int kPhcPi = 10, kPhcAvg = 15, kPhcPlayer = 10, kPhcUpdates = 30;   // pi_p at kPhcPi + p * kPhcPlayer, avg_p at kPhcAvg + ...
constexpr int kPhcLearn = 0, kPhcUniform = 1, kPhcFixed = 2;                   // = SOCCER_PHC_* (soccer_learners.hip asserts it)

struct PhcPopIO {
    double* tab;                        // [n][nS][32]
    double* alpha;                      // [n] every member's learning rate
    double* dscale;                     // [n] every member's factor on both deltas
    const double* decay;                // [n]
    const double* explor;               // [n]
    const double* gamma;                // [n]
    const double* delta_win;            // [n]
    const double* delta_lose;           // [n]
    const double* delta_decay;          // [n]
    unsigned long long* steps;
    unsigned int* misuse;               // the handle's sticky words
    int32_t nS;
    int32_t n_steps;                    // phc_pop_run_kernel: steps of this launch
    int32_t mode[2];                    // SOCCER_PHC_* of player A, player B
};

__device__ __forceinline__ void phc_pop_load_q(const double* at, double (&row)[10]) {
    const double2* p = reinterpret_cast<const double2*>(at);
#pragma unroll
    for (int k = 0; k < 5; ++k) { const double2 v = p[k]; row[2 * k] = v.x; row[2 * k + 1] = v.y; }
}

// pi_a | pi_b of one state's row (`at` = the row)
__device__ __forceinline__ void phc_pop_load_pi(const double* at, double (&pi)[10]) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const double* q = at + kPhcPi + p * kPhcPlayer;
        const double2 u = *reinterpret_cast<const double2*>(q), v = *reinterpret_cast<const double2*>(q + 2);
        pi[5 * p] = u.x; pi[5 * p + 1] = u.y; pi[5 * p + 2] = v.x; pi[5 * p + 3] = v.y; pi[5 * p + 4] = q[4];
    }
}

// avg_a | avg_b
__device__ __forceinline__ void phc_pop_load_avg(const double* at, double (&avg)[10]) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const double* q = at + kPhcAvg + p * kPhcPlayer;
        const double2 u = *reinterpret_cast<const double2*>(q + 1), v = *reinterpret_cast<const double2*>(q + 3);
        avg[5 * p] = q[0]; avg[5 * p + 1] = u.x; avg[5 * p + 2] = u.y; avg[5 * p + 3] = v.x; avg[5 * p + 4] = v.y;
    }
}

// step 5 of "learners, policy hill-climbing" for one player of one state, operation for operation as phc_update_kernel has
// it: pi and avg in registers, Q = the player's row AFTER the Q update, n = (double)updates[s] after its increment
__device__ __forceinline__ void phc_policy_step(double (&pi)[5], double (&avg)[5], const double (&Q)[5], double n, double delta_win,
                                                double delta_lose, double dscale) {
    double v = Q[0];
    int g = 0;
#pragma unroll
    for (int k = 1; k < 5; ++k)
        if (Q[k] > v) { v = Q[k]; g = k; }                       // the first index that attains it
    double ep = 0.0, ea = 0.0;
#pragma unroll
    for (int k = 0; k < 5; ++k) avg[k] = avg[k] + (pi[k] - avg[k]) / n;
#pragma unroll
    for (int k = 0; k < 5; ++k) { ep = ep + pi[k] * Q[k]; ea = ea + avg[k] * Q[k]; }
    const double d = ((ep > ea ? delta_win : delta_lose) * dscale) / 4.0;
    double moved = 0.0;
#pragma unroll
    for (int k = 0; k < 5; ++k)
        if (k != g) {
            const double m = pi[k] < d ? pi[k] : d;
            pi[k] = pi[k] - m;
            moved = moved + m;
        }
#pragma unroll
    for (int k = 0; k < 5; ++k)
        if (k == g) pi[k] = pi[k] + moved;
}

// steps 3-5 of one member on its one transition.  `at` = its row at s; q / pi = Q_a | Q_b and pi_a | pi_b at s, avg and upd
// what the row holds, nxt = Q_a | Q_b at s' as they were BEFORE this update.  Leaves the new q and pi in the caller's registers
// and stores everything that moved.
__device__ __forceinline__ void phc_pop_learn(const PhcPopIO& L, double* at, double (&q)[10], double (&pi)[10], double (&avg)[10],
                                              unsigned long long upd, const double (&nxt)[10], uint32_t a, uint32_t b, int32_t r,
                                              uint32_t term, double alpha, double gamma, double dwin, double dlose, double dscale) {
    double qa, qb;
    pop_learn(q, nxt, a, b, r, term, alpha, gamma, qa, qb);
    at[a] = qa; at[5u + b] = qb;
    upd += 1ull;
    *reinterpret_cast<unsigned long long*>(at + kPhcUpdates) = upd;
    const double n = (double)upd;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (L.mode[p] != kPhcLearn) continue;                   // wave-uniform
        double P[5], A[5], Q[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) { P[k] = pi[5 * p + k]; A[k] = avg[5 * p + k]; Q[k] = q[5 * p + k]; }
        phc_policy_step(P, A, Q, n, dwin, dlose, dscale);
#pragma unroll
        for (int k = 0; k < 5; ++k) pi[5 * p + k] = P[k];
        double2* const to = reinterpret_cast<double2*>(at + kPhcPi + p * kPhcPlayer);       // pi_p | avg_p: ten values
        to[0] = make_double2(P[0], P[1]); to[1] = make_double2(P[2], P[3]); to[2] = make_double2(P[4], A[0]);
        to[3] = make_double2(A[1], A[2]); to[4] = make_double2(A[3], A[4]);
    }
}

// a player's action from its 15-bit draw h: the null row table, or the thresholds of its own pi row at s — with the
// member's explor for a LEARN player, with 0.0 for a FIXED one (learner_thresholds: the host-computed table's bits)
__device__ __forceinline__ uint32_t phc_pop_draw(const PhcPopIO& L, int p, const double (&pi)[10], double explor, uint32_t h) {
    if (L.mode[p] == kPhcUniform) return (h * 5u) >> 15;                      // wave-uniform
    double row[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) row[k] = pi[5 * p + k];
    __attribute__((aligned(8))) uint16_t t[4];
    learner_thresholds(row, L.mode[p] == kPhcLearn ? explor : 0.0, t);
    return thresholds_not_above(*reinterpret_cast<const uint2*>(t), h);
}

template <bool SLIP, bool LUT_LDS>
__global__ __launch_bounds__(kBlock) void phc_pop_run_kernel(const KernelParams P, const PhcPopIO L) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    HistAcc<false> hist; hist.init(P);
    const Tables T = stage_tables<LUT_LDS>(P, smem);
    const unsigned long long tick0 = *P.tick_in;
    publish_tick(P, tick0, (unsigned long long)L.n_steps);
    if (blockIdx.x == 0 && threadIdx.x == 0) *L.steps += (unsigned long long)L.n_steps;
    bool any_frozen = false;
    for (unsigned long long g = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; g < P.n;
         g += (unsigned long long)gridDim.x * kBlock) {
        const unsigned long long i0 = P.first + g;                  // the lane, and the member
        LaneVec<1> S; S.load(P, i0);
        double* const tab = L.tab + (size_t)i0 * (size_t)L.nS * kPhcRow;
        double alpha = L.alpha[i0], dscale = L.dscale[i0];
        const double decay = L.decay[i0], explor = L.explor[i0], gamma = L.gamma[i0];
        const double dwin = L.delta_win[i0], dlose = L.delta_lose[i0], ddecay = L.delta_decay[i0];
        uint32_t s = obs_of(T, P, S.L[0].A, S.L[0].B, S.L[0].p);
        double q[10], pi[10];
        phc_pop_load_q(tab + (size_t)s * kPhcRow, q);
        phc_pop_load_pi(tab + (size_t)s * kPhcRow, pi);
        int32_t ret = 0; uint32_t eps = 0u, nonzero = 0u;
        for (int t = 0; t < L.n_steps; ++t) {
            const unsigned long long tick = tick0 + (unsigned long long)t;
            double* const at = tab + (size_t)s * kPhcRow;
            // used after the environment step only: issued here, dead at the end of the step
            double avg[10];
            phc_pop_load_avg(at, avg);
            const unsigned long long upd = *reinterpret_cast<const unsigned long long*>(at + kPhcUpdates);
            uint32_t words[1], awords[1];
            lane_words<1>(P, P.lane_offset + i0, block_tick<SLIP>(tick), 0u, words);
            lane_words<1>(P, P.lane_offset + i0, tick, 1u, awords);
            const Draw d = draw_from_word<SLIP>(words[0], tick);
            // two actions from one 32-bit word, 15 bits each (rollout_group)
            const uint32_t a = phc_pop_draw(L, 0, pi, explor, awords[0] & 0x7fffu);
            const uint32_t b = phc_pop_draw(L, 1, pi, explor, (awords[0] >> 16) & 0x7fffu);
            StepResult R;
            const bool frozen = lane_step<SLIP, true>(T, P, S.L[0], a, b, d, R);
            ret += R.reward; eps += R.finished; nonzero += (uint32_t)R.reward & 1u;
            any_frozen |= frozen;
            // (a lane parked in a goal tuple by soccer_set_state has s = 0: never a current state)
            const bool learn = !frozen && s != 0u;
            const uint32_t s2 = R.final_obs, sn = R.obs;
            double nxt[10], npi[10];
            if (learn) {
                phc_pop_load_q(tab + (size_t)s2 * kPhcRow, nxt);    // before the stores below: s' may be s
                phc_pop_load_pi(tab + (size_t)s2 * kPhcRow, npi);
                phc_pop_learn(L, at, q, pi, avg, upd, nxt, a, b, R.reward, R.term, alpha, gamma, dwin, dlose, dscale);
            }
            if (learn && sn == s2) {                                // the episode goes on: the rows at s' are the next rows at s
                if (s2 != s) {
#pragma unroll
                    for (int k = 0; k < 10; ++k) { q[k] = nxt[k]; pi[k] = npi[k]; }
                }                                                   // (s' == s: q and pi already hold what the update wrote)
            } else if (sn != s) {
                phc_pop_load_q(tab + (size_t)sn * kPhcRow, q);      // after a reset
                phc_pop_load_pi(tab + (size_t)sn * kPhcRow, pi);
            }
            s = sn;
            alpha = alpha * decay;
            dscale = dscale * ddecay;
        }
        S.store(P, i0);
        L.alpha[i0] = alpha; L.dscale[i0] = dscale;
        hist.add_totals(eps, ret, nonzero);
    }
    if (any_frozen) P.misuse[0] = 1u;
    hist.flush(P);
}

// soccer_wolf_population_update: steps 3-6 on the caller's transitions, transition i for member i
__global__ __launch_bounds__(kBlock) void phc_pop_update_kernel(const PhcPopIO L, long long n, const uint16_t* obs, const int8_t* act_a,
                                                                const int8_t* act_b, const int8_t* reward, const uint8_t* terminated,
                                                                const uint16_t* next_obs) {
    bool bad_act = false, bad_obs = false;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        const uint32_t s = obs[i], s2 = next_obs[i], a = (uint8_t)act_a[i], b = (uint8_t)act_b[i];
        const bool ba = a > 4u || b > 4u, bo = s == 0u || s >= (uint32_t)L.nS || s2 >= (uint32_t)L.nS;
        bad_act |= ba; bad_obs |= bo;
        const double alpha = L.alpha[i], dscale = L.dscale[i];
        if (!ba && !bo) {
            double* const tab = L.tab + (size_t)i * (size_t)L.nS * kPhcRow;
            double* const at = tab + (size_t)s * kPhcRow;
            double q[10], pi[10], avg[10], nxt[10];
            phc_pop_load_q(at, q); phc_pop_load_pi(at, pi); phc_pop_load_avg(at, avg);
            const unsigned long long upd = *reinterpret_cast<const unsigned long long*>(at + kPhcUpdates);
            phc_pop_load_q(tab + (size_t)s2 * kPhcRow, nxt);
            phc_pop_learn(L, at, q, pi, avg, upd, nxt, a, b, (int32_t)reward[i], terminated[i] != 0u ? 1u : 0u, alpha, L.gamma[i],
                          L.delta_win[i], L.delta_lose[i], dscale);
        }
        L.alpha[i] = alpha * L.decay[i];
        L.dscale[i] = dscale * L.delta_decay[i];
    }
    if (bad_act) L.misuse[1] = 1u;
    if (bad_obs) L.misuse[2] = 1u;
    if (blockIdx.x == 0 && threadIdx.x == 0) *L.steps += 1ull;
}

// creation: every member's Q_p = q_init on the live states and zero in row 0, pi = avg = 0.2, updates = 0, dscale = 1
__global__ __launch_bounds__(kBlock) void phc_pop_init_kernel(const PhcPopIO L, unsigned long long n, double q_init) {
    const unsigned long long per = (unsigned long long)L.nS * kPhcRow, cells = n * per;
    for (unsigned long long c = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; c < cells; c += (unsigned long long)gridDim.x * kBlock) {
        const unsigned slot = (unsigned)(c % kPhcRow);
        L.tab[c] = slot < 10u ? ((c % per) < (unsigned long long)kPhcRow ? 0.0 : q_init) : (slot < (unsigned)kPhcUpdates ? 0.2 : 0.0);
        if (c < n) L.dscale[c] = 1.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *L.steps = 0ull;
}

// A strided row copy: for `count` members from member `first` of dst, rows of five values from src (member m of the range at
// src + m * src_member, its state s at + s * src_row) into BOTH the pi and the avg row of dst's player (dst_slot = that
// player's pi slot).  soccer_wolf_population_adopt: src is another population's table at the slot to copy (strides nS * 32 and
// 32); creation: a dense [count][nS][5] staging block, or one [nS][5] policy with src_member = 0.
__global__ __launch_bounds__(kBlock) void phc_pop_adopt_kernel(double* dst, int dst_slot, const double* src, unsigned long long src_member,
                                                               unsigned long long src_row, unsigned long long first,
                                                               unsigned long long count, int32_t nS) {
    const unsigned long long rows = count * (unsigned long long)nS;
    for (unsigned long long c = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; c < rows; c += (unsigned long long)gridDim.x * kBlock) {
        const unsigned long long m = c / (unsigned long long)nS, s = c % (unsigned long long)nS;
        const double* const from = src + m * src_member + s * src_row;
        double* const to = dst + ((first + m) * (unsigned long long)nS + s) * kPhcRow + dst_slot;
#pragma unroll
        for (int k = 0; k < 5; ++k) { const double v = from[k]; to[k] = v; to[(kPhcAvg - kPhcPi) + k] = v; }
    }
}

// =================================================================================================
// a population of minimax-Q learners, a learner per lane (include/soccer_hip.h, "learners, a population of minimax-Q learners")
// =================================================================================================
// Member i is a soccer_minimax_q learner whose only actor is lane i.  Unlike the two populations above a member is NOT a
// thread: every learning step ends in solve_game5, whose GameWork (748 B, indexed at run time) has to live in LDS and whose
// pivoting would diverge across the members of a wave.  A member is a WAVE, one wave per workgroup: learner_update_kernel's
// shape (lanes 0..24 own the 25 cells, lane 0 solves from the wave's LDS slot), made persistent over the launch's steps.
// Table layout: member i's block is [nS][36] float64, one 288-byte, 16-byte aligned row per state:
//     0..24 Q[a * 5 + b]   25 V   26..30 pi_a   31..35 pi_b
// so a state's row is one coalesced load by lanes 0..35 (lanes 36..63 mirror slot 35 and never store), and a member's block
// is contiguous.  The wave holds the row at s in registers, one value per lane, as pop_run_kernel carries its row: it is the
// previous step's s' row while the episode goes on, already the updated and re-solved row when s' == s, loaded afresh only
// after a reset.  Everything that moved is stored straight away, so memory always holds what the registers hold and a launch
// boundary changes nothing.
// The environment step runs redundantly on all 64 lanes from wave-uniform inputs (the lane's state, the Philox words, the
// strategies broadcast with v_readlane) through lane_words / draw_from_word / lane_step / learner_thresholds, the functions
// every other learner calls; what decides a branch goes through v_readfirstlane, so the branches are scalar.  Lane 0 alone
// stores the lane state and feeds HistAcc.  The rule tables are read from global memory (the step kernel's placement): a
// workgroup of one wave that staged them to LDS would stage them once per member.
// Synchronisation: lanes exchange the Q row and the solver's answer through LDS inside the step loop.  With ONE wave per
// workgroup __syncthreads() is a wave-level barrier and cannot tie the loops of different members together; do not raise
// kMqBlock without replacing it.
constexpr int kMqBlock = 64;                        // one wave
constexpr int kMqRow = 36;                          // float64 slots per state
constexpr int kMqV = 25, kMqPiA = 26, kMqPiB = 31;
constexpr int kMqUniform = 0, kMqSelf = 1, kMqFixed = 2;   // = SOCCER_MQ_* (soccer_learners.hip asserts it)

struct MqPopIO {
    double* tab;                        // [n][nS][36]
    double* alpha;                      // [n] every member's learning rate
    const double* decay;                // [n]
    const double* explor;               // [n]
    const double* gamma;                // [n]
    const uint16_t* mix_b;              // SOCCER_MQ_FIXED: host-computed thresholds [nS][4] (mix_member = 0) or [n][nS][4]; else nullptr
    unsigned long long mix_member;      // uint16 elements between two members' threshold tables
    unsigned long long* steps;
    unsigned int* misuse;               // the handle's sticky words
    int32_t nS;
    int32_t n_steps;                    // mq_pop_run_kernel: steps of this launch
    int32_t opponent;                   // SOCCER_MQ_*
};

// the wave's LDS slot: the stage game, the solver's answer (V, pi_a, pi_b: slots 25..35 of the row) and its work memory
struct MqPopWork {
    double Q[25];
    double out[kMqRow - kMqV];
    GameWork w;
};

// slot `src` (a constant) of the row the wave holds, in every lane: two v_readlane, the result is wave-uniform
__device__ __forceinline__ double mq_row_slot(double val, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(val), src), hi = __builtin_amdgcn_readlane(__double2hiint(val), src);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ uint32_t mq_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// the action the 15-bit draw h takes from the strategy in slots first..first + 4 of the row, mixed with explor
__device__ __forceinline__ uint32_t mq_pop_draw(double val, int first, double explor, uint32_t h) {
    double pi[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) pi[k] = mq_row_slot(val, first + k);
    __attribute__((aligned(8))) uint16_t t[4];
    learner_thresholds(pi, explor, t);
    return thresholds_not_above(*reinterpret_cast<const uint2*>(t), h);
}

// step 5 for the state whose row the wave holds in `val` (`at` = that row in memory): lanes 0..24 hand Q[s] to lane 0, lane 0
// solves, lanes 25..35 take V, pi_a, pi_b into the row and store them.  Every lane of the wave calls it.
__device__ __forceinline__ void mq_pop_solve(double* at, double& val, int lane, MqPopWork* W) {
    if (lane < kMqV) W->Q[lane] = val;
    __syncthreads();
    if (lane == 0) {
        double v = 0.0, x[5], y[5];
        solve_game5(W->Q, &W->w, &v, x, y);
        W->out[0] = v;
#pragma unroll
        for (int k = 0; k < 5; ++k) { W->out[kMqPiA - kMqV + k] = x[k]; W->out[kMqPiB - kMqV + k] = y[k]; }
    }
    __syncthreads();
    if (lane >= kMqV && lane < kMqRow) { val = W->out[lane - kMqV]; at[lane] = val; }
}

// steps 3-5 of one member on its one transition (s live, a / b in 0..4; all arguments wave-uniform but val and lane): v_next =
// V[s'] as it was BEFORE this update.  c = 1, so the mean target is the sample's own, on the learners' grid.
__device__ __forceinline__ void mq_pop_learn(double* at, double& val, double v_next, uint32_t a, uint32_t b, int32_t r, uint32_t term,
                                             double alpha, double gamma, int lane, MqPopWork* W) {
    const long long SV = term ? 0ll : (long long)rint(v_next * kVqScale);
    const double m = (double)r + gamma * ((double)SV * kVqInv);
    if ((uint32_t)lane == a * 5u + b) { val = val + alpha * (m - val); at[lane] = val; }
    mq_pop_solve(at, val, lane, W);
}

template <bool SLIP>
__global__ __launch_bounds__(kMqBlock) void mq_pop_run_kernel(const KernelParams P, const MqPopIO L) {
    __shared__ MqPopWork W;
    HistAcc<false> hist; hist.init(P);
    Tables T; T.lut = P.lut; T.nc = P.next_cell; T.isd = P.isd;
    const int lane = (int)threadIdx.x;
    const int slot = lane < kMqRow ? lane : kMqRow - 1;
    const unsigned long long tick0 = *P.tick_in;
    publish_tick(P, tick0, (unsigned long long)L.n_steps);
    if (blockIdx.x == 0 && threadIdx.x == 0) *L.steps += (unsigned long long)L.n_steps;
    bool any_frozen = false;
    for (unsigned long long g = blockIdx.x; g < P.n; g += gridDim.x) {      // a wave serves members g, g + gridDim.x, ... in turn
        const unsigned long long i0 = P.first + g;                  // the lane, and the member
        LaneVec<1> S; S.load(P, i0);
        double* const tab = L.tab + (size_t)i0 * (size_t)L.nS * kMqRow;
        const uint16_t* const mix = L.mix_b ? L.mix_b + (size_t)i0 * (size_t)L.mix_member : nullptr;
        double alpha = L.alpha[i0];
        const double decay = L.decay[i0], explor = L.explor[i0], gamma = L.gamma[i0];
        uint32_t s = mq_uniform(obs_of(T, P, S.L[0].A, S.L[0].B, S.L[0].p));
        double val = tab[(size_t)s * kMqRow + slot];
        int32_t ret = 0; uint32_t eps = 0u, nonzero = 0u;
        for (int t = 0; t < L.n_steps; ++t) {
            const unsigned long long tick = tick0 + (unsigned long long)t;
            const StepDraws w = step_draws<SLIP>(P, i0, tick);
            const uint32_t a = mq_uniform(mq_pop_draw(val, kMqPiA, explor, w.ha));
            uint32_t b;
            if (L.opponent == kMqUniform) {                         // wave-uniform
                b = (w.hb * 5u) >> 15;
            } else if (L.opponent == kMqSelf) {
                b = mq_pop_draw(val, kMqPiB, explor, w.hb);
            } else {
                b = thresholds_not_above(*reinterpret_cast<const uint2*>(mix + 4u * s), w.hb);
            }
            b = mq_uniform(b);
            StepResult R;
            const bool frozen = mq_uniform(lane_step<SLIP, true>(T, P, S.L[0], a, b, w.d, R) ? 1u : 0u) != 0u;
            ret += R.reward; eps += R.finished; nonzero += (uint32_t)R.reward & 1u;
            any_frozen |= frozen;
            // (a lane parked in a goal tuple by soccer_set_state has s = 0: never a current state)
            const bool learn = !frozen && s != 0u;
            const uint32_t s2 = mq_uniform(R.final_obs), sn = mq_uniform(R.obs);
            double nxt = 0.0;
            if (learn) {
                nxt = tab[(size_t)s2 * kMqRow + slot];              // before the stores below: s' may be s
                mq_pop_learn(tab + (size_t)s * kMqRow, val, mq_row_slot(nxt, kMqV), a, b, (int32_t)mq_uniform((uint32_t)R.reward),
                             mq_uniform(R.term), alpha, gamma, lane, &W);
            }
            if (learn && sn == s2) {                                // the episode goes on: the row at s' is the next row at s
                if (s2 != s) val = nxt;                             // (s' == s: val already holds what the update and the solve wrote)
            } else if (sn != s) {
                val = tab[(size_t)sn * kMqRow + slot];              // after a reset
            }
            s = sn;
            alpha = alpha * decay;
        }
        if (lane == 0) {
            S.store(P, i0);
            L.alpha[i0] = alpha;
            hist.add_totals(eps, ret, nonzero);
        }
    }
    if (any_frozen && lane == 0) P.misuse[0] = 1u;
    hist.flush(P);
}

// soccer_minimax_q_population_update: steps 3-6 on the caller's transitions, transition i for member i, a wave per member
__global__ __launch_bounds__(kMqBlock) void mq_pop_update_kernel(const MqPopIO L, long long n, const uint16_t* obs, const int8_t* act_a,
                                                                 const int8_t* act_b, const int8_t* reward, const uint8_t* terminated,
                                                                 const uint16_t* next_obs) {
    __shared__ MqPopWork W;
    const int lane = (int)threadIdx.x;
    const int slot = lane < kMqRow ? lane : kMqRow - 1;
    bool bad_act = false, bad_obs = false;
    for (long long i = blockIdx.x; i < n; i += gridDim.x) {
        const uint32_t s = mq_uniform(obs[i]), s2 = mq_uniform(next_obs[i]);
        const uint32_t a = mq_uniform((uint8_t)act_a[i]), b = mq_uniform((uint8_t)act_b[i]);
        const bool ba = a > 4u || b > 4u, bo = s == 0u || s >= (uint32_t)L.nS || s2 >= (uint32_t)L.nS;
        bad_act |= ba; bad_obs |= bo;
        const double alpha = L.alpha[i];
        if (!ba && !bo) {
            double* const tab = L.tab + (size_t)i * (size_t)L.nS * kMqRow;
            double* const at = tab + (size_t)s * kMqRow;
            double val = at[slot];
            const double v_next = tab[(size_t)s2 * kMqRow + kMqV];
            mq_pop_learn(at, val, v_next, a, b, (int32_t)mq_uniform((uint32_t)(int32_t)reward[i]), terminated[i] != 0u ? 1u : 0u, alpha,
                         L.gamma[i], lane, &W);
        }
        if (lane == 0) L.alpha[i] = alpha * L.decay[i];
    }
    if (lane == 0) {
        if (bad_act) L.misuse[1] = 1u;
        if (bad_obs) L.misuse[2] = 1u;
        if (blockIdx.x == 0) *L.steps += 1ull;
    }
}

// soccer_minimax_q_population_load with Q alone: every live state of members first .. first + count - 1 is re-solved (MODE 2
// of learner_update_kernel), a wave per state
__global__ __launch_bounds__(kMqBlock) void mq_pop_solve_kernel(const MqPopIO L, unsigned long long first, unsigned long long count) {
    __shared__ MqPopWork W;
    const int lane = (int)threadIdx.x;
    const int slot = lane < kMqRow ? lane : kMqRow - 1;
    const unsigned long long live = (unsigned long long)L.nS - 1ull, rows = count * live;
    for (unsigned long long c = blockIdx.x; c < rows; c += gridDim.x) {
        const unsigned long long m = c / live, s = 1ull + c % live;
        double* const at = L.tab + ((first + m) * (unsigned long long)L.nS + s) * kMqRow;
        double val = at[slot];
        mq_pop_solve(at, val, lane, &W);
    }
}

// creation: every member's Q = V = q_init on the live states and zero in row 0, uniform strategies (set, not solved)
__global__ __launch_bounds__(kBlock) void mq_pop_init_kernel(const MqPopIO L, unsigned long long n, double q_init) {
    const unsigned long long per = (unsigned long long)L.nS * kMqRow, cells = n * per;
    for (unsigned long long c = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; c < cells; c += (unsigned long long)gridDim.x * kBlock)
        L.tab[c] = (unsigned)(c % kMqRow) <= (unsigned)kMqV ? ((c % per) < (unsigned long long)kMqRow ? 0.0 : q_init) : 0.2;
    if (blockIdx.x == 0 && threadIdx.x == 0) *L.steps = 0ull;
}

// =================================================================================================
// a population of opponent-modelling Q-learners, a learner per lane (include/soccer_hip.h, "learners, a population of
// opponent-modelling Q-learners")
// =================================================================================================
// pop_run_kernel's shape: a thread owns lane i and member i, nothing is shared between threads, no atomics, no second launch.
// Its argument block is PopIO with Q = the members' rows.
// Table layout: member i's block is [nS][2][32] 8-byte slots — player A's 256-byte row, then player B's, are the 512
// adjacent, 256-byte aligned bytes a step needs at s.  Per player:
//     0..24 Q[own * 5 + other] (float64)   25..29 C[other] (uint64)   30 V (float64)   31 g (uint64)
// so (V, g) is one 16-byte load, and a member's block is contiguous: a range of members is one copy.
// V and g are kept in the row (derived by om_derive, the one function every kernel here calls, and stored whenever Q or C
// of the row moved) so that a step's dependent chain is short: acting needs g_p[s] alone, carried in a register — it is
// what the (V, g) load at s' of the previous step brought while the episode goes on, what om_learn just derived when
// s' == s, and loaded only after a reset; the bootstrap needs V_p[s'] alone, that one 16-byte load per player.  The full
// row at s (25 Q + 5 C) is needed only to derive again after the update: its address is known at the top of the step, so
// player A's row is asked for before the environment step; player B's row is loaded when A's is done, so that one player's
// 30 values are live at a time.  The cell, the count and (V, g) are stored straight away: memory always holds what the
// registers hold, a launch boundary changes nothing, and a thread's later load at s' == s sees its own store.
// Actions and cells are COMPARED, never used as subscripts of the register rows (pop_learn's rule): 0 bytes of scratch.
constexpr int kOmPlayer = 32;                       // slots per player and state
constexpr int kOmRow = 2 * kOmPlayer;               // slots per state
constexpr int kOmC = 25, kOmV = 30;                 // a player's counts; its (V, g) pair

struct OmRow {
    double Q[25];                       // [own][other]
    unsigned long long C[5];            // [other]
};

__device__ __forceinline__ void om_load_row(const double* at, OmRow& row) {
    const double2* p = reinterpret_cast<const double2*>(at);
    double v[30];
#pragma unroll
    for (int k = 0; k < 15; ++k) { const double2 x = p[k]; v[2 * k] = x.x; v[2 * k + 1] = x.y; }
#pragma unroll
    for (int k = 0; k < 25; ++k) row.Q[k] = v[k];
#pragma unroll
    for (int k = 0; k < 5; ++k) row.C[k] = (unsigned long long)__double_as_longlong(v[kOmC + k]);
}

// THE derived values of one (player, state): the greedy answer g to the empirical frequencies of the other player's
// actions, and its value V (the header's expression, operation for operation; the build does not contract)
__device__ __forceinline__ void om_derive(const OmRow& row, double& V, uint32_t& g) {
    const unsigned long long n = row.C[0] + row.C[1] + row.C[2] + row.C[3] + row.C[4];
    double w[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) w[k] = n > 0ull ? (double)row.C[k] : 1.0;
    const double N = n > 0ull ? (double)n : 5.0;
    double best = 0.0;
    g = 0u;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        double W = w[0] * row.Q[5 * a];
#pragma unroll
        for (int k = 1; k < 5; ++k) W = W + w[k] * row.Q[5 * a + k];
        if (a == 0 || W > best) { best = W; g = (uint32_t)a; }              // the first index that attains it
    }
    const double v = best / N;
    V = v < -1.0 ? -1.0 : (v > 1.0 ? 1.0 : v);
}

__device__ __forceinline__ void om_store_derived(double* at, double V, uint32_t g) {
    *reinterpret_cast<double2*>(at + kOmV) = make_double2(V, __longlong_as_double((long long)g));
}

// the (V, g) pair of one player's row
__device__ __forceinline__ void om_load_derived(const double* at, double& V, uint32_t& g) {
    const double2 x = *reinterpret_cast<const double2*>(at + kOmV);
    V = x.x; g = (uint32_t)__double_as_longlong(x.y);
}

// steps 4-5 of one player of one member on its one transition: `at` = the player's row at s in memory, `row` = that row in
// registers, own / other = the two actions as this player sees them, r = its own reward, v_next = its V[s'] as it was BEFORE
// this update.  Moves and stores the cell, the count and (V, g); hands the new g back.
__device__ __forceinline__ void om_learn(double* at, OmRow& row, uint32_t own, uint32_t other, int32_t r, uint32_t term, double v_next,
                                         double alpha, double gamma, uint32_t& g) {
    const long long SV = term ? 0ll : (long long)rint(v_next * kVqScale);
    const double m = (double)r + gamma * ((double)SV * kVqInv);
    const uint32_t cell = own * 5u + other;
    double old = row.Q[0];
#pragma unroll
    for (int k = 1; k < 25; ++k) old = (uint32_t)k == cell ? row.Q[k] : old;
    const double moved = old + alpha * (m - old);
#pragma unroll
    for (int k = 0; k < 25; ++k) row.Q[k] = (uint32_t)k == cell ? moved : row.Q[k];
    unsigned long long c = 0ull;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        row.C[k] += (uint32_t)k == other ? 1ull : 0ull;
        c = (uint32_t)k == other ? row.C[k] : c;
    }
    at[cell] = moved;
    reinterpret_cast<unsigned long long*>(at)[kOmC + other] = c;
    double V;
    om_derive(row, V, g);
    om_store_derived(at, V, g);
}

// a player's action from its 15-bit draw h: the null row table, the shared fixed rows, or epsilon-greedy on onehot(g)
__device__ __forceinline__ uint32_t om_pop_draw(const PopIO& L, int p, uint32_t g, uint32_t s, double explor, uint32_t h) {
    if (L.mode[p] == kPopUniform) return (h * 5u) >> 15;                       // wave-uniform
    uint2 th;
    if (L.mode[p] == kPopGreedy) {
        double pi[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) pi[k] = (uint32_t)k == g ? 1.0 : 0.0;
        __attribute__((aligned(8))) uint16_t t[4];
        learner_thresholds(pi, explor, t);
        th = *reinterpret_cast<const uint2*>(t);
    } else {
        th = *reinterpret_cast<const uint2*>(L.mix[p] + 4u * s);
    }
    return (h >= (th.x & 0xffffu)) + (h >= (th.x >> 16)) + (h >= (th.y & 0xffffu)) + (h >= (th.y >> 16));
}

template <bool SLIP, bool LUT_LDS>
__global__ __launch_bounds__(kBlock) void om_pop_run_kernel(const KernelParams P, const PopIO L) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    HistAcc<false> hist; hist.init(P);
    const Tables T = stage_tables<LUT_LDS>(P, smem);
    const unsigned long long tick0 = *P.tick_in;
    publish_tick(P, tick0, (unsigned long long)L.n_steps);
    if (blockIdx.x == 0 && threadIdx.x == 0) *L.steps += (unsigned long long)L.n_steps;
    bool any_frozen = false;
    for (unsigned long long g = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; g < P.n;
         g += (unsigned long long)gridDim.x * kBlock) {
        const unsigned long long i0 = P.first + g;                  // the lane, and the member
        LaneVec<1> S; S.load(P, i0);
        double* const tab = L.Q + (size_t)i0 * (size_t)L.nS * kOmRow;
        double alpha = L.alpha[i0];
        const double decay = L.decay[i0], explor = L.explor[i0], gamma = L.gamma[i0];
        uint32_t s = obs_of(T, P, S.L[0].A, S.L[0].B, S.L[0].p);
        double unused;
        uint32_t ga, gb;                                            // g_A[s], g_B[s]
        om_load_derived(tab + (size_t)s * kOmRow, unused, ga);
        om_load_derived(tab + (size_t)s * kOmRow + kOmPlayer, unused, gb);
        int32_t ret = 0; uint32_t eps = 0u, nonzero = 0u;
        for (int t = 0; t < L.n_steps; ++t) {
            const unsigned long long tick = tick0 + (unsigned long long)t;
            double* const at = tab + (size_t)s * kOmRow;
            OmRow row;
            om_load_row(at, row);                                   // player A's row at s: wanted only after the step
            uint32_t words[1], awords[1];
            lane_words<1>(P, P.lane_offset + i0, block_tick<SLIP>(tick), 0u, words);
            lane_words<1>(P, P.lane_offset + i0, tick, 1u, awords);
            const Draw d = draw_from_word<SLIP>(words[0], tick);
            // two actions from one 32-bit word, 15 bits each (rollout_group)
            const uint32_t a = om_pop_draw(L, 0, ga, s, explor, awords[0] & 0x7fffu);
            const uint32_t b = om_pop_draw(L, 1, gb, s, explor, (awords[0] >> 16) & 0x7fffu);
            StepResult R;
            const bool frozen = lane_step<SLIP, true>(T, P, S.L[0], a, b, d, R);
            ret += R.reward; eps += R.finished; nonzero += (uint32_t)R.reward & 1u;
            any_frozen |= frozen;
            // (a lane parked in a goal tuple by soccer_set_state has s = 0: never a current state)
            const bool learn = !frozen && s != 0u;
            const uint32_t s2 = R.final_obs, sn = R.obs;
            uint32_t ga2 = 0u, gb2 = 0u;
            if (learn) {
                double va2, vb2;                                    // before the stores below: s' may be s
                om_load_derived(tab + (size_t)s2 * kOmRow, va2, ga2);
                om_load_derived(tab + (size_t)s2 * kOmRow + kOmPlayer, vb2, gb2);
                om_learn(at, row, a, b, R.reward, R.term, va2, alpha, gamma, ga);
                om_load_row(at + kOmPlayer, row);
                om_learn(at + kOmPlayer, row, b, a, -R.reward, R.term, vb2, alpha, gamma, gb);
            }                                                       // (ga, gb are g at s as the update left it)
            if (sn != s) {
                if (learn && sn == s2) {                            // the episode goes on: the pair at s' is the next pair at s
                    ga = ga2; gb = gb2;
                } else {                                            // after a reset
                    om_load_derived(tab + (size_t)sn * kOmRow, unused, ga);
                    om_load_derived(tab + (size_t)sn * kOmRow + kOmPlayer, unused, gb);
                }
            }
            s = sn;
            alpha = alpha * decay;
        }
        S.store(P, i0);
        L.alpha[i0] = alpha;
        hist.add_totals(eps, ret, nonzero);
    }
    if (any_frozen) P.misuse[0] = 1u;
    hist.flush(P);
}

// soccer_om_population_update: steps 3-6 on the caller's transitions, transition i for member i
__global__ __launch_bounds__(kBlock) void om_pop_update_kernel(const PopIO L, long long n, const uint16_t* obs, const int8_t* act_a,
                                                               const int8_t* act_b, const int8_t* reward, const uint8_t* terminated,
                                                               const uint16_t* next_obs) {
    bool bad_act = false, bad_obs = false;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        const uint32_t s = obs[i], s2 = next_obs[i], a = (uint8_t)act_a[i], b = (uint8_t)act_b[i];
        const bool ba = a > 4u || b > 4u, bo = s == 0u || s >= (uint32_t)L.nS || s2 >= (uint32_t)L.nS;
        bad_act |= ba; bad_obs |= bo;
        const double alpha = L.alpha[i];
        if (!ba && !bo) {
            double* const tab = L.Q + (size_t)i * (size_t)L.nS * kOmRow;
            double* const at = tab + (size_t)s * kOmRow;
            const uint32_t term = terminated[i] != 0u ? 1u : 0u;
            const int32_t r = (int32_t)reward[i];
            double va2, vb2;                                        // before the stores below: s' may be s
            uint32_t g;
            om_load_derived(tab + (size_t)s2 * kOmRow, va2, g);
            om_load_derived(tab + (size_t)s2 * kOmRow + kOmPlayer, vb2, g);
            OmRow row;
            om_load_row(at, row);
            om_learn(at, row, a, b, r, term, va2, alpha, L.gamma[i], g);
            om_load_row(at + kOmPlayer, row);
            om_learn(at + kOmPlayer, row, b, a, -r, term, vb2, alpha, L.gamma[i], g);
        }
        L.alpha[i] = alpha * L.decay[i];
    }
    if (bad_act) L.misuse[1] = 1u;
    if (bad_obs) L.misuse[2] = 1u;
    if (blockIdx.x == 0 && threadIdx.x == 0) *L.steps += 1ull;
}

// creation: every member's Q_p = q_init on the live states, row 0 and every count zero, (V, g) derived; a thread per
// (member, state, player) row
__global__ __launch_bounds__(kBlock) void om_pop_init_kernel(const PopIO L, unsigned long long n, double q_init) {
    const unsigned long long rows = n * (unsigned long long)L.nS * 2ull;
    for (unsigned long long c = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; c < rows; c += (unsigned long long)gridDim.x * kBlock) {
        double* const at = L.Q + c * kOmPlayer;
        const double q = (c / 2ull) % (unsigned long long)L.nS == 0ull ? 0.0 : q_init;
        OmRow row;
#pragma unroll
        for (int k = 0; k < 25; ++k) { row.Q[k] = q; at[k] = q; }
#pragma unroll
        for (int k = 0; k < 5; ++k) { row.C[k] = 0ull; reinterpret_cast<unsigned long long*>(at)[kOmC + k] = 0ull; }
        double V; uint32_t g;
        om_derive(row, V, g);
        om_store_derived(at, V, g);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *L.steps = 0ull;
}

// soccer_om_population_load: (V, g) of every row of members first .. first + count - 1 follow what was loaded
__global__ __launch_bounds__(kBlock) void om_pop_derive_kernel(const PopIO L, unsigned long long first, unsigned long long count) {
    const unsigned long long per = (unsigned long long)L.nS * 2ull, rows = count * per;
    for (unsigned long long c = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; c < rows; c += (unsigned long long)gridDim.x * kBlock) {
        double* const at = L.Q + (first * per + c) * kOmPlayer;
        OmRow row;
        om_load_row(at, row);
        double V; uint32_t g;
        om_derive(row, V, g);
        om_store_derived(at, V, g);
    }
}

// =================================================================================================
// a population of regret matchers, a learner per lane (include/soccer_hip.h, "learners, a population of regret matchers")
// =================================================================================================
// phc_pop_run_kernel's shape: a thread owns lane i and member i, the lane and the rows of the current state in registers over
// the launch's steps, no atomics, no second launch.  lane_words / draw_from_word / lane_step / learner_thresholds are the same
// functions the other learners call.
// Table layout: the hill-climbers' [nS][32] float64 row with two columns reread, one 256-byte aligned row per state:
//     0..4 Q_a   5..9 Q_b   10..14 R_a   15..19 Z_a   20..24 R_b   25..29 Z_b   30 updates (uint64)   31 pad
// so phc_pop_load_q / _pi / _avg load Q, R and Z, and everything a step needs at s is two cache lines.  The policy is NOT
// stored: rm_policy recomputes it from R (five divides per player and state instead of a third cache line; which is cheaper is
// unmeasured).  A FIXED player's rows live in a buffer of their own, [n or 1][nS][5], read only on the wave-uniform
// FIXED branch: at s for the draw and at s' for the bootstrap.
// What a step carries: Q_a, Q_b, R_a, R_b at s (the next draw and, as the previous step's s' rows, the bootstrap).  Z and updates
// at s are used only after the environment step: their loads are issued at the top of the step and nothing of them lives
// across steps.  Everything is unrolled over the five actions with the action index COMPARED, never used as a subscript: the
// rows stay in registers (0 bytes of scratch).
constexpr int kRmR = kPhcPi, kRmZ = kPhcAvg, kRmPlayer = kPhcPlayer, kRmUpdates = kPhcUpdates;   // R_p at kRmR + p * kRmPlayer, Z_p at kRmZ + ...

struct RmPopIO {
    double* tab;                        // [n][nS][32]
    double* alpha;                      // [n] every member's learning rate
    const double* decay;                // [n]
    const double* explor;               // [n]
    const double* gamma;                // [n]
    const double* fixed[2];             // a FIXED player's rows [nS][5] (fixed_member = 0) or [n][nS][5]; else nullptr
    unsigned long long fixed_member[2]; // float64 elements between two members' rows
    unsigned long long* steps;
    unsigned int* misuse;               // the handle's sticky words
    int32_t nS;
    int32_t n_steps;                    // rm_pop_run_kernel: steps of this launch
    int32_t mode[2];                    // SOCCER_PHC_* of player A, player B
    int32_t plus, linear;               // regrets floored at 0; a step's policy weighed by the visit count
};

// policy(p, s) of the header for a LEARN player: the normalised positive part of its regrets R (rows of ten: both players')
__device__ __forceinline__ void rm_policy(const double (&R)[10], int p, double (&pi)[10]) {
    double pos[5], tot = 0.0;
#pragma unroll
    for (int k = 0; k < 5; ++k) { pos[k] = R[5 * p + k] > 0.0 ? R[5 * p + k] : 0.0; tot = tot + pos[k]; }
#pragma unroll
    for (int k = 0; k < 5; ++k) pi[5 * p + k] = tot > 0.0 ? pos[k] / tot : 0.2;
}

// policy(p, s) for both players: R = the regrets at s, s = the state (a FIXED player's row is loaded from its own buffer)
__device__ __forceinline__ void rm_policies(const RmPopIO& L, const double* const (&fixed)[2], const double (&R)[10], uint32_t s,
                                            double (&pi)[10]) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (L.mode[p] == kPhcLearn) {                              // wave-uniform
            rm_policy(R, p, pi);
        } else if (L.mode[p] == kPhcUniform) {
#pragma unroll
            for (int k = 0; k < 5; ++k) pi[5 * p + k] = 0.2;
        } else {
            const double* const row = fixed[p] + (size_t)s * 5;
#pragma unroll
            for (int k = 0; k < 5; ++k) pi[5 * p + k] = row[k];
        }
    }
}

// a player's action from its 15-bit draw h: the null row table, or the thresholds of its policy row at s — with the member's
// explor for a LEARN player, with 0.0 for a FIXED one (phc_pop_draw's rule)
__device__ __forceinline__ uint32_t rm_pop_draw(const RmPopIO& L, int p, const double (&pi)[10], double explor, uint32_t h) {
    if (L.mode[p] == kPhcUniform) return (h * 5u) >> 15;                      // wave-uniform
    double row[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) row[k] = pi[5 * p + k];
    __attribute__((aligned(8))) uint16_t t[4];
    learner_thresholds(row, L.mode[p] == kPhcLearn ? explor : 0.0, t);
    return thresholds_not_above(*reinterpret_cast<const uint2*>(t), h);
}

// steps 2-4 of one member on its one transition.  `at` = its row at s; q / R = Q_a | Q_b and R_a | R_b at s, Z and upd what
// the row holds, pi = both policies at s; nq and npi = Q_a | Q_b and both policies at s' as they were BEFORE this update.
// Leaves the new q and R in the caller's registers and stores everything that moved.
__device__ __forceinline__ void rm_pop_learn(const RmPopIO& L, double* at, double (&q)[10], double (&R)[10], double (&Z)[10],
                                             unsigned long long upd, const double (&pi)[10], const double (&nq)[10],
                                             const double (&npi)[10], uint32_t a, uint32_t b, int32_t r, uint32_t term, double alpha,
                                             double gamma) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {                                   // step 2: the bootstrap is the value of the player's own policy
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 5; ++k) v = v + npi[5 * p + k] * nq[5 * p + k];
        v = term ? 0.0 : v;
        const double m = (double)(p ? -r : r) + gamma * v;         // player B's own reward
        const uint32_t act = p ? b : a;
        double moved_q = 0.0;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const double old = q[5 * p + k];
            const double moved = old + alpha * (m - old);
            q[5 * p + k] = (uint32_t)k == act ? moved : old;
            moved_q = (uint32_t)k == act ? moved : moved_q;
        }
        at[(p ? 5u : 0u) + act] = moved_q;
    }
    upd += 1ull;                                                    // step 3
    *reinterpret_cast<unsigned long long*>(at + kRmUpdates) = upd;
    const double w = L.linear ? (double)upd : 1.0;
#pragma unroll
    for (int p = 0; p < 2; ++p) {                                   // step 4
        if (L.mode[p] != kPhcLearn) continue;                       // wave-uniform
        double u = 0.0, r5[5], z5[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) u = u + pi[5 * p + k] * q[5 * p + k];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            double x = R[5 * p + k] + (q[5 * p + k] - u);
            if (L.plus) x = x > 0.0 ? x : 0.0;
            r5[k] = x; R[5 * p + k] = x;
            z5[k] = Z[5 * p + k] + w * pi[5 * p + k];
        }
        double2* const to = reinterpret_cast<double2*>(at + kRmR + p * kRmPlayer);          // R_p | Z_p: ten values
        to[0] = make_double2(r5[0], r5[1]); to[1] = make_double2(r5[2], r5[3]); to[2] = make_double2(r5[4], z5[0]);
        to[3] = make_double2(z5[1], z5[2]); to[4] = make_double2(z5[3], z5[4]);
    }
}

template <bool SLIP, bool LUT_LDS>
__global__ __launch_bounds__(kBlock) void rm_pop_run_kernel(const KernelParams P, const RmPopIO L) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    HistAcc<false> hist; hist.init(P);
    const Tables T = stage_tables<LUT_LDS>(P, smem);
    const unsigned long long tick0 = *P.tick_in;
    publish_tick(P, tick0, (unsigned long long)L.n_steps);
    if (blockIdx.x == 0 && threadIdx.x == 0) *L.steps += (unsigned long long)L.n_steps;
    bool any_frozen = false;
    for (unsigned long long g = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; g < P.n;
         g += (unsigned long long)gridDim.x * kBlock) {
        const unsigned long long i0 = P.first + g;                  // the lane, and the member
        LaneVec<1> S; S.load(P, i0);
        double* const tab = L.tab + (size_t)i0 * (size_t)L.nS * kPhcRow;
        // (a null pointer plus zero for a player that is not FIXED: never read)
        const double* const fixed[2] = {L.fixed[0] + (size_t)i0 * (size_t)L.fixed_member[0], L.fixed[1] + (size_t)i0 * (size_t)L.fixed_member[1]};
        double alpha = L.alpha[i0];
        const double decay = L.decay[i0], explor = L.explor[i0], gamma = L.gamma[i0];
        uint32_t s = obs_of(T, P, S.L[0].A, S.L[0].B, S.L[0].p);
        double q[10], R[10];
        phc_pop_load_q(tab + (size_t)s * kPhcRow, q);
        phc_pop_load_pi(tab + (size_t)s * kPhcRow, R);
        int32_t ret = 0; uint32_t eps = 0u, nonzero = 0u;
        for (int t = 0; t < L.n_steps; ++t) {
            const unsigned long long tick = tick0 + (unsigned long long)t;
            double* const at = tab + (size_t)s * kPhcRow;
            // used after the environment step only: issued here, dead at the end of the step
            double Z[10];
            phc_pop_load_avg(at, Z);
            const unsigned long long upd = *reinterpret_cast<const unsigned long long*>(at + kRmUpdates);
            double pi[10];
            rm_policies(L, fixed, R, s, pi);
            uint32_t words[1], awords[1];
            lane_words<1>(P, P.lane_offset + i0, block_tick<SLIP>(tick), 0u, words);
            lane_words<1>(P, P.lane_offset + i0, tick, 1u, awords);
            const Draw d = draw_from_word<SLIP>(words[0], tick);
            // two actions from one 32-bit word, 15 bits each (rollout_group)
            const uint32_t a = rm_pop_draw(L, 0, pi, explor, awords[0] & 0x7fffu);
            const uint32_t b = rm_pop_draw(L, 1, pi, explor, (awords[0] >> 16) & 0x7fffu);
            StepResult Rs;
            const bool frozen = lane_step<SLIP, true>(T, P, S.L[0], a, b, d, Rs);
            ret += Rs.reward; eps += Rs.finished; nonzero += (uint32_t)Rs.reward & 1u;
            any_frozen |= frozen;
            // (a lane parked in a goal tuple by soccer_set_state has s = 0: never a current state)
            const bool learn = !frozen && s != 0u;
            const uint32_t s2 = Rs.final_obs, sn = Rs.obs;
            double nq[10], nR[10];
            if (learn) {
                phc_pop_load_q(tab + (size_t)s2 * kPhcRow, nq);     // before the stores below: s' may be s
                phc_pop_load_pi(tab + (size_t)s2 * kPhcRow, nR);
                double npi[10];
                rm_policies(L, fixed, nR, s2, npi);
                rm_pop_learn(L, at, q, R, Z, upd, pi, nq, npi, a, b, Rs.reward, Rs.term, alpha, gamma);
            }
            if (learn && sn == s2) {                                // the episode goes on: the rows at s' are the next rows at s
                if (s2 != s) {
#pragma unroll
                    for (int k = 0; k < 10; ++k) { q[k] = nq[k]; R[k] = nR[k]; }
                }                                                   // (s' == s: q and R already hold what the update wrote)
            } else if (sn != s) {
                phc_pop_load_q(tab + (size_t)sn * kPhcRow, q);      // after a reset
                phc_pop_load_pi(tab + (size_t)sn * kPhcRow, R);
            }
            s = sn;
            alpha = alpha * decay;
        }
        S.store(P, i0);
        L.alpha[i0] = alpha;
        hist.add_totals(eps, ret, nonzero);
    }
    if (any_frozen) P.misuse[0] = 1u;
    hist.flush(P);
}

// soccer_regret_population_update: steps 1-5 on the caller's transitions, transition i for member i
__global__ __launch_bounds__(kBlock) void rm_pop_update_kernel(const RmPopIO L, long long n, const uint16_t* obs, const int8_t* act_a,
                                                               const int8_t* act_b, const int8_t* reward, const uint8_t* terminated,
                                                               const uint16_t* next_obs) {
    bool bad_act = false, bad_obs = false;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        const uint32_t s = obs[i], s2 = next_obs[i], a = (uint8_t)act_a[i], b = (uint8_t)act_b[i];
        const bool ba = a > 4u || b > 4u, bo = s == 0u || s >= (uint32_t)L.nS || s2 >= (uint32_t)L.nS;
        bad_act |= ba; bad_obs |= bo;
        const double alpha = L.alpha[i];
        if (!ba && !bo) {
            double* const tab = L.tab + (size_t)i * (size_t)L.nS * kPhcRow;
            double* const at = tab + (size_t)s * kPhcRow;
            const double* const fixed[2] = {L.fixed[0] + (size_t)i * (size_t)L.fixed_member[0], L.fixed[1] + (size_t)i * (size_t)L.fixed_member[1]};
            double q[10], R[10], Z[10], pi[10], nq[10], nR[10], npi[10];
            phc_pop_load_q(at, q); phc_pop_load_pi(at, R); phc_pop_load_avg(at, Z);
            const unsigned long long upd = *reinterpret_cast<const unsigned long long*>(at + kRmUpdates);
            phc_pop_load_q(tab + (size_t)s2 * kPhcRow, nq);
            phc_pop_load_pi(tab + (size_t)s2 * kPhcRow, nR);
            rm_policies(L, fixed, R, s, pi);
            rm_policies(L, fixed, nR, s2, npi);
            rm_pop_learn(L, at, q, R, Z, upd, pi, nq, npi, a, b, (int32_t)reward[i], terminated[i] != 0u ? 1u : 0u, alpha, L.gamma[i]);
        }
        L.alpha[i] = alpha * L.decay[i];
    }
    if (bad_act) L.misuse[1] = 1u;
    if (bad_obs) L.misuse[2] = 1u;
    if (blockIdx.x == 0 && threadIdx.x == 0) *L.steps += 1ull;
}

// creation: every member's Q_p = q_init on the live states and zero in row 0, R = Z = 0, updates = 0
__global__ __launch_bounds__(kBlock) void rm_pop_init_kernel(const RmPopIO L, unsigned long long n, double q_init) {
    const unsigned long long per = (unsigned long long)L.nS * kPhcRow, cells = n * per;
    for (unsigned long long c = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; c < cells; c += (unsigned long long)gridDim.x * kBlock)
        L.tab[c] = (unsigned)(c % kPhcRow) < 10u && (c % per) >= (unsigned long long)kPhcRow ? q_init : 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) *L.steps = 0ull;
}

}  // namespace soccer
