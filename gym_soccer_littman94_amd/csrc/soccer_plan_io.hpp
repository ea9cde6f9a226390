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

// best responses to, and evaluations of, a batch of mixed policies over the same lists (response_sweep_kernel)
enum ResponseMode : int32_t { kRespondB = 0, kRespondA = 1, kEvalPair = 2 };   // B answers x, A answers y, the pair (x, y)

struct ResponseIO {
    MinimaxIO mm;                    // offset, list, gamma, theta, nS; the kernel points mm.V at its policy's V_{k-1}
    const double* x;                 // [n][nS][5] player A's policies (kRespondB, kEvalPair)
    const double* y;                 // [n][nS][5] player B's policies (kRespondA, kEvalPair)
    const double* V;                 // [n][nS] V_{k-1}
    double* V_out;                   // [n][nS] V_k
    double* Qr;                      // [n][nS][5] (not kEvalPair)
    int32_t* br;                     // [n][nS]    (not kEvalPair)
    unsigned long long* delta;       // this sweep's word of policy 0; policy i's is word_stride words further per policy
    const unsigned long long* prev;  // likewise the previous sweep's (never NULL)
    int32_t word_stride;
};

// the payoff matrix of n_a x n_b mixed policies (soccer_cross_play): evaluations like kEvalPair's, transposed — a lane owns a
// pair, V and the words are laid out [..][stride] with the pass's pairs along the fastest axis
struct CrossIO {
    const int32_t* offset; const PlanEntry* list;   // MinimaxIO's lists
    const double* x;                 // [n_a][nS][5] player A's policies, row 0 of each zeroed
    const double* y;                 // [n_b][nS][5] player B's
    const double* V;                 // [nS][stride] V_{k-1}
    double* V_out;                   // [nS][stride] V_k
    unsigned long long* delta;       // [stride] this sweep's word of every pair of the pass
    const unsigned long long* prev;  // [stride] the previous sweep's
    double gamma, theta;
    int32_t nS, n_b;
    int32_t stride, pairs;           // pairs of the pass, and that number rounded up to whole waves
    int32_t first, last;             // matrix index i * n_b + j of the pass's pair 0, and of the matrix's last pair
};

// between two batches of sweeps (cross_batch_kernel): each pair's stopping sweep from the batch's words, the words reset
struct CrossBatchIO {
    unsigned long long* words;       // [n_words][stride]; row 0 is the sweep before the batch's first
    int32_t* done_at;                // [stride] the pair's stopping sweep, 0 while it is open
    int32_t* open;                   // the kernel adds the number of pairs still open
    double theta;
    int32_t stride, pairs, n_words;
    int32_t k0, nb;                  // the batch's first sweep and its length; nb == 0: before the first batch
};

// after the last batch (cross_finish_kernel, cross_values_kernel): every pair from the V buffer of its own parity
struct CrossFinishIO {
    const double* V[2];              // [nS][stride] each
    const int32_t* done_at;          // [stride]
    double* payoff;                  // [stride] the mean of V over the initial states
    int32_t* iterations;             // [stride]
    double* values;                  // [pairs][nS] (cross_values_kernel only)
    int32_t isd[4];                  // the initial states' observation indices in ISD order
    int32_t n_isd, nS, stride, pairs, max_sweeps;
};

// match outcomes of n_a x n_b mixed policies (soccer_match_outcomes): three value vectors per pair, the win probabilities of
// A and of B and the game's length.  match_sweep_kernel takes a CrossIO whose V and V_out are [nS][3][stride] and whose gamma
// is the continuation probability, cross_batch_kernel its CrossBatchIO; after the last batch (match_finish_kernel,
// match_values_kernel):
struct MatchFinishIO {
    const double* V[2];              // [nS][3][stride] each
    const int32_t* done_at;          // [stride]
    double* kickoff;                 // [3][stride] the mean of each channel over the initial states
    int32_t* iterations;             // [stride]
    double* values;                  // [pairs][3][nS] (match_values_kernel only)
    int32_t isd[4];                  // the initial states' observation indices in ISD order
    int32_t n_isd, nS, stride, pairs, max_sweeps;
};

// state occupancy of n_a x n_b mixed policies (soccer_occupancy): the expected discounted number of visits to every state.
// The sweep runs the transition relation backwards, over in-lists (soccer_inlists.hpp builds them from MinimaxIO's lists):
// one in-entry, 16 bytes = one dwordx4 load, is the probability of the out-entry it mirrors and that entry's key
// s * 25 + a * 5 + b; in-lists are padded to kPlanPad with (prob 0.0, source key 0) entries.
struct __attribute__((aligned(16))) InEntry { double prob; int32_t source_key; int32_t pad; };

// occupancy_sweep_kernel; cross_batch_kernel takes its CrossBatchIO between the batches, cross_values_kernel a CrossFinishIO
struct OccupancyIO {
    const int32_t* in_offset; const InEntry* in_list;   // [nS + 1], the in-lists
    const double* xT;                // [nS][5][n_a] player A's policies, the policy along the fastest axis, row 0 zeroed
    const double* yT;                // [nS][5][n_b] player B's
    const double* D;                 // [nS][stride] D_{k-1}
    double* D_out;                   // [nS][stride] D_k
    unsigned long long* delta;       // [stride] this sweep's word of every pair of the pass
    const unsigned long long* prev;  // [stride] the previous sweep's
    double c, theta, mu;             // the continuation probability; 1.0 / n_isd
    int32_t isd[4];                  // the initial states' observation indices
    int32_t n_isd, nS, n_a, n_b;
    int32_t stride, pairs;
    int32_t first, last;             // as CrossIO's
};

// the caller's policies [n][nS][5] -> [nS][5][n], row 0 as zeros (occupancy_transpose_kernel)
struct OccupancyPolicyIO {
    const double* pol; double* polT;
    int32_t n, rows;                 // rows = nS * 5
};

// after the last batch (occupancy_finish_kernel): a thread per (pair, sum) from the D buffer of the pair's own parity
struct OccupancyFinishIO {
    const double* D[2];              // [nS][stride] each
    const int32_t* done_at;          // [stride]
    const double* features;          // [n_f][nS]
    double* length;                  // [stride] (NULL: not asked for)
    double* expect;                  // [pairs][n_f]
    int32_t* iterations;             // [stride]
    int32_t nS, stride, pairs, max_sweeps, n_f;
};

// exact policy gradients of n_a x n_b mixed policies (soccer_policy_gradient): a pass's V is solved as cross-play's and its D
// as the occupancy's, over the same pairs at one stride; then (action_values_kernel) one more backup from every pair's final V,
// mixed with the other side's policy
struct ActionValuesIO {
    const int32_t* offset; const PlanEntry* list;   // MinimaxIO's lists
    const double* x;                 // [n_a][nS][5] player A's policies, row 0 of each zeroed
    const double* y;                 // [n_b][nS][5] player B's
    const double* V[2];              // [nS][stride] each; a pair's final V is in the buffer of its own parity
    const int32_t* done_at;          // [stride] the V solve's stopping sweeps
    double* Qa;                      // [nS][5][stride] Q_a[s][a] = sum_b y[s][b] * q[a][b]
    double* Qb;                      // [nS][5][stride] Q_b[s][b] = sum_a x[s][a] * q[a][b]
    double gamma;
    int32_t nS, n_b;
    int32_t stride, pairs;
    int32_t first, last;             // as CrossIO's
    int32_t max_sweeps;
};

// gradient_reduce_kernel: a pass's pairs added to one side's running sums, in ascending order of the other side's index
struct GradientReduceIO {
    const double* D[2];              // [nS][stride] each; a pair's final D is in the buffer of its own parity
    const int32_t* done_at;          // [stride] the D solve's stopping sweeps
    const double* Q;                 // [nS][5][stride] this side's action values
    const double* w;                 // the OTHER side's weights
    double* grad;                    // [n_own][nS][5] the running sums, carried from pass to pass
    double* reach;                   // [n_own][nS]
    int32_t side;                    // 0: player A's (a row i of the matrix, summed over j), 1: player B's (a column j, over i)
    int32_t n_a, n_b, nS;
    int32_t stride, pairs, first, max_sweeps;
};

// gradient_normalize_kernel, after the last pass: grad[r][a] = reach[r] > 0.0 ? grad[r][a] / reach[r] : 0.0
struct GradientNormalizeIO {
    double* grad; const double* reach;
    int64_t rows;                    // n_own * nS
};

// gradient_step_kernel (soccer_gradient_play_run): one projected step of every row of both players' policies
struct GradientStepIO {
    double* pol;                     // [n_a + n_b][nS][5] the resident policies, player A's first
    double* prev;                    // [n_a + n_b][nS][5] the previous step's gradients
    const double* grad;              // [n_a + n_b][nS][5] this step's
    double eta_a, eta_b, optimism;
    int64_t rows_a, rows;            // n_a * nS, (n_a + n_b) * nS
    int32_t nS, first_step;
};

// a pass of n_a x n_b zero-sum matrix games (soccer_solve_meta_games): the record of a game, and what every kernel of
// soccer_metagame_kernels.hpp is given
constexpr int kMetaRec = 8;
enum MetaRecWord : int {
    kMetaClosed = 0,                 // 0 while the game pivots, 1 once it has stopped
    kMetaStatus = 1,                 // 1 saddle point, 3 stopped at the cap, -1 finished (0 or 2 once the bracket is known)
    kMetaPivots = 2,
    kMetaCol = 3, kMetaRow = 4,      // the pivot the next update applies
    kMetaIStar = 5, kMetaJStar = 6,  // the saddle point
};
struct MetaIO {
    const double* A;                 // [games][n_a][n_b] the caller's matrices
    double* T;                       // [games][rows][stride] the tableaux (the global path; the LDS path keeps them in LDS)
    double* prow;                    // [games][stride] the scaled pivot row
    double* fcol;                    // [games][rows] the pivot column before the update: every row's factor
    int32_t* basis;                  // [games][n_a]
    int32_t* rec;                    // [games][kMetaRec]
    double* amax;                    // [games] max |A|
    double* x; double* y;            // [games][n_a], [games][n_b]
    double* value; double* lo; double* hi;          // [games]
    int32_t* pivots; int32_t* status;               // [games]
    int32_t* open;                   // meta_count_kernel adds the games still pivoting
    int32_t n_a, n_b;
    int32_t rows, cols, stride;      // n_a + 1, n_a + n_b + 2, cols rounded up to an odd number
    int32_t max_pivots, games;
};

}  // namespace soccer
