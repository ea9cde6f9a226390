// soccer_plan_io.hpp — the planners' argument blocks.  Plain structs: the handle caches one of each (soccer_handle.hpp),
// the kernels that read them are in soccer_planner_kernels.hpp.
#pragma once
#include <stdint.h>

namespace soccer {

enum PlanMode : int32_t { kPlanVI = 0, kPlanEval = 1, kPlanImprove = 2, kPlanPI = 3, kPlanMPI = 4, kPlanEvalDense = 5 };

// one list entry, 16 bytes = one dwordx4 load.  Lists are padded to a multiple of kPlanPad entries with
// (prob 0, next 0, done) entries, which add an exact +-0 to the running sum, so the planner loops can fetch
// kPlanPad entries per wait without changing a bit of the result.
struct __attribute__((aligned(16))) PlanEntry { double prob; int32_t next_done; float reward; };   // next | done << 31
constexpr int kPlanPad = 4;

struct PlanIO {
    // P[s][a] lists in the reference's order (:167-293), CSR by (state, learner action): offset[nS*5 + 1];
    // reward is the learner's (+-1, +-0)
    const int32_t* offset; const PlanEntry* list;
    // rows of Pmat / Rmat (:280-291): per (state, action) the next states in ascending index with their
    // accumulated probability (the dense dot's order), and the expected reward
    const int32_t* m_offset; const PlanEntry* m_list; const double* m_R;
    double* V; double* newV; double* Q; int32_t* pi;
    int32_t* counters;          // [0] outer iterations, [1] sweeps, [2] 1 = stopped by max_sweeps
    int32_t nS, mode, max_sweeps, k;
    double theta, gamma, threshold;
};

struct MinimaxIO {
    const int32_t* offset;           // [nS * 25 + 1] CSR by (state, joint action a * 5 + b)
    const PlanEntry* list;           // padded to kPlanPad like the single-agent lists; reward is player A's
    const double* V;                 // V_{k-1}
    double* V_out;                   // V_k
    double* Q;                       // [nS][5][5]
    double* pi_a; double* pi_b;      // [nS][5]
    unsigned long long* delta;       // this sweep's word (NULL: no reduction)
    const unsigned long long* prev;  // the previous sweep's word (NULL: always run)
    double gamma, theta;
    int32_t nS;
};

}  // namespace soccer
