// soccer_learner_kernels.hpp — the minimax-Q learner (Littman 1994): learner_act_kernel, learner_reduce_kernel,
// learner_update_kernel, learner_init_kernel.
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
template <bool SLIP, bool LUT_LDS>
__global__ __launch_bounds__(kBlock) void learner_act_kernel(const KernelParams P, const LearnerIO L) {
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
        uint32_t words[1], awords[1];
        lane_words<1>(P, P.lane_offset + i0, block_tick<SLIP>(tick), 0u, words);
        lane_words<1>(P, P.lane_offset + i0, tick, 1u, awords);
        const Draw d = draw_from_word<SLIP>(words[0], tick);
        // two actions from one 32-bit word, 15 bits each (rollout_group): the number of thresholds <= the draw
        const uint32_t ha = awords[0] & 0x7fffu, hb = (awords[0] >> 16) & 0x7fffu;
        uint32_t a, b = (hb * 5u) >> 15;
        {
            const uint2 th = *reinterpret_cast<const uint2*>(L.mix_a + 4u * s_now);
            a = (ha >= (th.x & 0xffffu)) + (ha >= (th.x >> 16)) + (ha >= (th.y & 0xffffu)) + (ha >= (th.y >> 16));
        }
        if (L.mix_b) {
            const uint2 th = *reinterpret_cast<const uint2*>(L.mix_b + 4u * s_now);
            b = (hb >= (th.x & 0xffffu)) + (hb >= (th.x >> 16)) + (hb >= (th.y & 0xffffu)) + (hb >= (th.y >> 16));
        }
        StepResult R;
        const bool frozen = lane_step<SLIP, true>(T, P, S.L[0], a, b, d, R);
        S.store(P, i0);
        hist.add_totals(R.finished, R.reward, (uint32_t)R.reward & 1u);
        any_frozen |= frozen;
        // (a lane parked in a goal tuple by soccer_set_state has s = 0: never a current state)
        if (!frozen && s_now != 0u) learner_accumulate(L, s_now, a, b, R.reward, R.term, R.final_obs);
    }
    if (any_frozen) P.misuse[0] = 1u;
    hist.flush(P);
}

// soccer_minimax_q_update: step 3 on the caller's transitions, a thread each
__global__ __launch_bounds__(kBlock) void learner_reduce_kernel(const LearnerIO L, long long n, const uint16_t* obs, const int8_t* act_a,
                                                                const int8_t* act_b, const int8_t* reward, const uint8_t* terminated,
                                                                const uint16_t* next_obs) {
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

}  // namespace soccer
