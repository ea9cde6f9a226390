// soccer_handle.hpp — what the translation units of libsoccer_hip.so share on the host side: the handle, error reporting,
// and the few functions one unit needs from another.  Internal: not installed, not part of the C ABI (include/soccer_hip.h).
//
//   soccer_hip.hip       create / destroy, seed / tick, reset, state, staging, one-environment calls, statistics, timers, graphs
//   soccer_step.hip      batched_step*
//   soccer_rollout.hip   batched_rollout*
//   soccer_planners.hip  the transition table, the single-agent planners, minimax value iteration, best responses, the matrix-game solver
//   soccer_pairs.hip     the pair evaluators on one host skeleton: cross-play, match outcomes, state occupancy, policy gradients, and gradient play
//   soccer_metagame.hip  soccer_solve_meta_games: the maximin mixtures of n_a x n_b matrix games
//   soccer_learners.hip  the nine kinds of learners on one host skeleton: minimax-Q, independent Q, WoLF-PHC, a population of each, a
//                        population of opponent-modelling Q-learners, and regret matchers in both forms
//   soccer_comm.hip      the RCCL wrapper (host code only)
//
// Every unit carries its own code object: a kernel is instantiated, launched and given its attributes (hipFuncSetAttribute)
// in ONE unit only — see the kernel headers named in soccer_kernels.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/soccer_hip.h"
#include "soccer_inlists.hpp"
#include "soccer_kernels.hpp"
#include "soccer_plan_io.hpp"
#include "soccer_rules.hpp"

#pragma GCC visibility push(hidden)      // nothing below is an export of the library

using namespace soccer;

// error text into the handle (or, without one, into the calling thread's slot that soccer_last_error(NULL) reads); returns `code`
int fail(soccer_handle* h, int code, const char* fmt, ...);

#define HIP_TRY(h, expr)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail((h), e_ == hipErrorOutOfMemory ? SOCCER_E_NOMEM : SOCCER_E_HIP,          \
                        "%s failed: %s", #expr, hipGetErrorString(e_));                          \
    } while (0)

template <typename T>
static inline bool aligned(const T* p, size_t a) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) % a) == 0; }

template <class T> static inline T* off(T* p, unsigned long long lanes) { return p ? p + lanes : nullptr; }   // NULL stays NULL

// The one owner of memory the library allocates for itself: device memory (hipMalloc) and pinned host memory
// (hipHostMalloc), each block freed once by clear(), which the destructor calls.  An allocation hands its typed pointer
// back through an out-parameter; whoever keeps that pointer (the handle's d_* members, the planners' argument blocks)
// does not own it.  The handle has one for what lives as long as it does, the planners' cached lists have their own
// (dropped by a failed build and by whatever invalidates the lists), a call's temporaries a local one.
struct OwnedBufs {
    struct Buf { void* ptr; bool pinned; };
    enum PinnedFlags : unsigned { kPinned = hipHostMallocDefault, kPinnedMapped = hipHostMallocMapped };   // (mapped: the device addresses it too)
    const char* what;                       // for the error message
    std::vector<Buf> bufs;
    bool ready = false;                     // set by a builder once every buffer holds its content
    explicit OwnedBufs(const char* owner) : what(owner) {}
    OwnedBufs(const OwnedBufs&) = delete;
    OwnedBufs& operator=(const OwnedBufs&) = delete;
    ~OwnedBufs() { clear(); }

    template <class T>
    int alloc(soccer_handle* h, size_t count, T** out) { return take(h, hipMalloc(out, bytes<T>(count)), false, out); }
    template <class T>
    int alloc_pinned(soccer_handle* h, size_t count, PinnedFlags flags, T** out) { return take(h, hipHostMalloc(out, bytes<T>(count), flags), true, out); }
    template <class T>
    int upload(soccer_handle* h, const std::vector<T>& v, const T** out) {
        T* d = nullptr;
        if (int rc = alloc(h, v.size(), &d)) return rc;
        if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
            return fail(h, SOCCER_E_HIP, "upload of %s failed", what);
        *out = d;
        return SOCCER_OK;
    }
    // gives one block back early (a buffer whose set-up failed half way)
    void release(void* p) {
        for (size_t i = 0; i < bufs.size(); ++i) if (bufs[i].ptr == p) { drop(bufs[i]); bufs.erase(bufs.begin() + i); return; }
    }
    void clear() {
        for (const Buf& b : bufs) drop(b);
        bufs.clear(); ready = false;
    }

private:
    template <class T> static size_t bytes(size_t count) { return count ? count * sizeof(T) : 1; }
    static void drop(const Buf& b) { (void)(b.pinned ? hipHostFree(b.ptr) : hipFree(b.ptr)); }
    template <class T>
    int take(soccer_handle* h, hipError_t e, bool pinned, T** out) {
        if (e != hipSuccess) {
            *out = nullptr;
            return e == hipErrorOutOfMemory ? fail(h, SOCCER_E_NOMEM, "out of %s memory for %s", pinned ? "pinned host" : "device", what)
                                            : fail(h, SOCCER_E_HIP, "allocation for %s failed: %s", what, hipGetErrorString(e));
        }
        bufs.push_back(Buf{*out, pinned});
        return SOCCER_OK;
    }
};

struct soccer_graph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    uint64_t ticks = 0;       // ticks consumed by one replay
    int start_slot = 0;       // tick slot the first captured launch reads
    bool stamped = false;     // soccer_timer_start / _mark were captured: a replay writes stamp slots 0 and 1
    int32_t kernel_nodes = 0;   // soccer_graph_info: kernel nodes the batched_* calls recorded (launch parts one by one; not the stamps, not the tick-move node)
    int64_t steps_fused = 0;    // ... captured steps that went into multi-step launches
    int32_t fused_launches = 0; // ... and the runs they formed
};

// Captured steps that have not been launched yet (soccer_step.hip): consecutive batched_step calls of one capture whose rows
// are evenly spaced are one rollout, and are recorded as one when the run ends (flush_pending).  `first` is the run's first
// step by value; the strides are fixed by the second step.
struct PendingRun {
    soccer_step_args first{};
    int64_t len = 0;                        // steps in the run (0: none pending)
    int64_t act_stride = 0, out_stride = 0; // elements between consecutive steps (len >= 2)
};

struct Learner;                             // soccer_learners.hip: what the nine kinds of learners have in common

// What solve_pass (soccer_pairs.hip) works on: the buffers of one solve over the pairs of a pass, the pairs along the fastest axis.
struct PassBufs {
    double* buf[2] = {nullptr, nullptr};    // [rows][stride] the iterate, double-buffered across sweeps
    unsigned long long* words = nullptr;    // [kMinimaxBatch + 1][stride] per-sweep, per-pair max |change| (bits)
    int32_t* done = nullptr;                // [stride] each pair's stopping sweep
    int32_t* open = nullptr;                // the number of open pairs after a batch
    int stride = 0;
};

// The buffer family of one pair evaluator: a call's policies and one pass's buffers.  `policies`, `pass.stride` and
// `has_values` say what is held; pair_buffers (soccer_pairs.hip) is the only one to allocate here.
struct PairBufs {
    OwnedBufs bufs;
    PassBufs pass;                          // rows: nS (soccer_match_outcomes: kMatchChannels * nS, the channels of a state side by side)
    double* pol = nullptr;                  // [policies][nS][5] as the caller gives them: player A's policies, then player B's
    double* polT = nullptr;                 // [nS][5][n_a] player A's with the policy along the fastest axis, then [nS][5][n_b] (where the sweep reads in-lists)
    int32_t* iter = nullptr;                // [stride] the sweep counts as they are returned (max_sweeps for an open pair)
    double* values = nullptr;               // [stride][width] a pass's iterate in the caller's order (has_values: allocated)
    int policies = 0; bool has_values = false;
    explicit PairBufs(const char* owner) : bufs(owner) {}
};
struct CrossOwn { double* payoff = nullptr; };                          // [stride]
struct MatchOwn { double* kickoff = nullptr; };                         // [kMatchChannels][stride]
struct OccupancyOwn {
    double* length = nullptr;               // [stride]
    double* expect = nullptr;               // [pairs of the pass][n_f], room for [stride][SOCCER_OCC_MAX_FEATURES]
    double* features = nullptr;             // [SOCCER_OCC_MAX_FEATURES][nS] the caller's
};
struct GradientOwn {                        // the family's own pass is V's; its values buffer takes V, D, q_a or q_b in turn
    PassBufs D;                             // the occupancy's solve over the same pairs: buffers and stopping sweeps of its own, V's words and count
    double* Q = nullptr;                    // [2][nS][5][stride] Q_a, then Q_b: the ten action-value planes
    double* payoff = nullptr;               // [stride]
    double* grad = nullptr;                 // [policies][nS][5] the running sums: grad_a, then grad_b
    double* reach = nullptr;                // [policies][nS]
    double* w = nullptr;                    // [policies] w_a, then w_b
};

struct soccer_handle {
    soccer_config cfg{};
    Rules rules;
    KernelParams P{};
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // what soccer_create allocates and what is allocated on first use and lives as long as the handle; the typed members
    // below point into it and own nothing
    OwnedBufs bufs{"the handle"};
    uint16_t* d_lut = nullptr; uint32_t* d_nc = nullptr; uint32_t* d_isd = nullptr;
    int8_t* d_policy[2] = {nullptr, nullptr};
    unsigned long long* d_tick = nullptr;   // two slots, 128 B apart
    unsigned long long* d_hist = nullptr;
    unsigned int* d_misuse = nullptr;       // device alias of misuse_host
    unsigned int* misuse_host = nullptr;    // pinned + mapped: kernels store to it only when a frozen lane is stepped (rare),
                                            // the host reads it without a copy
    uint8_t* d_state = nullptr;             // one allocation holding the SoA state streams back to back
    size_t state_stride = 0;                // bytes between consecutive streams
    int state_streams = 6;                  // 3: the packed layout (KernelParams::state_layout == kStatePacked), 6: wide
    uint8_t* stage_dev = nullptr;           // staging for the host-pointer entry points
    uint8_t* stage_host = nullptr;          // pinned
    bool mapped = false;                    // SOCCER_F_HOST_MAPPED: d_state and the staging block are pinned host memory
    size_t stage_bytes = 0;
    int tick_slot = 0;                      // slot the NEXT launch reads
    uint64_t tick = 0;                      // host mirror of the device tick
    bool slip = false, lut_lds = false;
    size_t smem_bytes = 0;
    int E = 4;
    int grid_cap = 2048;
    bool capturing = false;
    uint64_t capture_ticks = 0;
    int capture_calls = 0;
    int capture_start_slot = 0;
    PendingRun run;                         // captured steps not launched yet; dropped with the capture
    bool graph_fuse = true;                 // SOCCER_GRAPH_FUSE=0 (A/B runs): every captured step is a launch of its own
    int capture_kernels = 0;                // kernel nodes the batched_* calls of this capture recorded (note_kernel)
    int64_t capture_steps_fused = 0; int capture_fused_launches = 0;
    int n_cu = 256;
    size_t lds_limit = 64 * 1024;           // hipDeviceProp_t::sharedMemPerBlockOptin: what a workgroup may be given (160 KB on gfx950)
    uint4* d_sub = nullptr;                 // integer slip thresholds (KernelParams::sub)
    uint4* rec_host = nullptr; uint4* rec_dev = nullptr; uint32_t rec_seq = 0;   // soccer_step_scalar's mapped result record
    // byte-parallel step (soccer_swar.hpp)
    swar::Consts swar_c{}; bool swar_ok = false;
    swar::SlipConsts slip_c{}; bool slip_swar_ok = false;   // integer slip selection usable by the byte-parallel kernels
    uint32_t* d_slip_lut = nullptr;         // SlipTables::lut + T for the table form of the selection (when lut_ok)
    uint32_t* d_slip_step_lut = nullptr;    // SlipTables::lut_step + T: the single step's table (when lut_step_ok)
    size_t hist_slots = kHistSlots;         // per-wave histogram slots (a power of two; see soccer_create)
    bool timer_stamped = false; int wall_clock_khz = 100000;   // captured timers: see stamp_kernel
    bool capture_stamped = false;           // THIS capture recorded soccer_timer_start / _mark (what soccer_graph::stamped is copied from)
    bool stamp_poll = false;                // soccer_timer_read may watch the closing stamp of the last soccer_graph_launch change ...
    unsigned long long stamp_prev = 0;      // ... from this value (what the slot held when the replay was enqueued)
    unsigned long long swar_launch_lanes = kSwarLaunchLanes;   // lanes per step_kernel_swar / rollout_swar_kernel launch (SOCCER_SWAR_LAUNCH_LANES: tests of the split)
    int rollout_pref = 0;                   // SOCCER_ROLLOUT=1 (A/B runs, tests of the fallback): never the byte-parallel rollout
    soccer_rollout_shape_info last_rollout{};   // soccer_rollout_shape: what batched_rollout_ex last launched (lds_limit is filled in on read)
    SlipF64* d_slip_f64 = nullptr;          // SLIPM == 3: nominal float64 slip thresholds (step_kernel_swar with caller-supplied uniforms)
    uint32_t* d_worklist = nullptr;         // ... and the groups it leaves to the exact walk: [n / 4] indices, the count and the
                                            // tail's statistics behind them (worklist_count)
    unsigned long long* d_traj_hist = nullptr;   // soccer_trajectory_returns: u64[3] the kernel adds into
    void* comm = nullptr; int comm_world = 0, comm_rank = 0;   // soccer_comm_init: the RCCL communicator of this handle's device
    unsigned long long* d_comm_scratch = nullptr;   // 64 B for the small reductions (barrier, histogram, clocks)
    PlanIO plan{};                          // cached planner lists (single-agent mode), see build_plan
    OwnedBufs plan_bufs{"the planner lists"};   // dropped when the policy changes (soccer_set_policy)
    MinimaxIO mm{};                         // cached two-player lists and buffers of the minimax planners, see build_minimax
    double* mm_V[2] = {nullptr, nullptr};   // V double-buffered across sweeps
    unsigned long long* mm_words = nullptr; // [kMinimaxBatch + 1] per-sweep max |V_k - V_{k-1}| (bits)
    OwnedBufs mm_bufs{"the minimax planner"};
    // soccer_best_response / soccer_evaluate_policies: buffers for br_cap policies (br_pairs: and a second policy block),
    // allocated on first use and again when a larger batch comes, see response_buffers
    double* br_pol[2] = {nullptr, nullptr}; // [br_cap][nS][5] the fixed side's policies; [1]: player B's of a pair
    double* br_V[2] = {nullptr, nullptr};   // [br_cap][nS] V double-buffered across sweeps
    double* br_Qr = nullptr;                // [br_cap][nS][5]
    int32_t* br_arg = nullptr;              // [br_cap][nS]
    unsigned long long* br_words = nullptr; // [br_cap][kMinimaxBatch + 1] per-policy, per-sweep max |V_k - V_{k-1}| (bits)
    int br_cap = 0; bool br_pairs = false;
    OwnedBufs br_bufs{"the best-response solver"};
    // the pair evaluators (soccer_pairs.hip): a buffer family each, allocated on first use and again when a call needs more
    // policies, a longer pass or the values for the first time (pair_buffers); what only one of them has sits beside it
    PairBufs cross{"the cross-play solver"};          CrossOwn cross_own;
    PairBufs match{"the match-outcome solver"};       MatchOwn match_own;      // kMatchChannels rows per state in the iterate and the values
    PairBufs occupancy{"the occupancy solver"};       OccupancyOwn occupancy_own;
    PairBufs gradient{"the policy-gradient solver"};  GradientOwn gradient_own;    // (soccer_gradient_play_run steps along gradient_own.grad)
    // soccer_occupancy and soccer_policy_gradient: the two-player lists the other way round (build_inlists, once per handle
    // like the lists they derive from)
    const int32_t* in_offset = nullptr;     // [nS + 1]
    const InEntry* in_list = nullptr;       // padded to kPlanPad
    OwnedBufs in_lists{"the occupancy solver's in-lists"};
    std::vector<soccer_gradient_play*> gradient_players;       // soccer_gradient_play_create's, freed with the handle
    // soccer_solve_meta_games: one pass's buffers, allocated on first use and again when a pass needs more of any, see meta_buffers
    double* mg_A = nullptr;                 // [games][n_a][n_b] the caller's matrices
    double* mg_T = nullptr;                 // [games][n_a + 1][stride] the tableaux (the global path only)
    double* mg_x = nullptr; double* mg_y = nullptr;   // [games][n_a], [games][n_b]
    double* mg_fcol = nullptr; double* mg_prow = nullptr;   // [games][n_a + 1], [games][stride] the side buffers of a pivot
    int32_t* mg_basis = nullptr;            // [games][n_a]
    double* mg_scal = nullptr;              // [4][games] value, lo, hi, max |A|
    int32_t* mg_int = nullptr;              // [games][kMetaRec] the records, then [games] pivots, [games] status, the open count
    size_t mg_need[5] = {0, 0, 0, 0, 0};    // what the buffers hold, in meta_need's order
    OwnedBufs mg_bufs{"the meta-game solver"};
    std::vector<Learner*> learners;         // soccer_*_create of soccer_learners.hip: the learners and populations of every kind that
                                            // were not destroyed (freed with the handle, learners_release)
    std::string err;

    soccer_handle() = default;
    soccer_handle(const soccer_handle&) = delete;
    soccer_handle& operator=(const soccer_handle&) = delete;
    ~soccer_handle();                       // soccer_hip.hip: waits for the stream, then gives everything back
};

// the handle's host-mapped block: dwords 0 / 1 / 2 the sticky misuse words (frozen, action, observation), from byte 64 on SOCCER_STAMP_SLOTS u64 clock stamps,
// ONE PER 64-BYTE LINE: a line the host has written or is polling costs the device a coherence round trip to write, and a
// stamp kernel's store must complete before the next kernel starts — with the opening and the closing stamp of a captured
// timer in one line (and the host clearing the closing one before every replay) the opening stamp's kernel boundary took
// microseconds longer and inflated the region it opens
constexpr size_t kStampStride = 8;          // in u64
constexpr size_t kMappedBytes = 64 + 8 * kStampStride * SOCCER_STAMP_SLOTS;

// the tick lives in device memory so that a captured graph advances it on every replay: launch j
// reads slot (j & 1) and writes slot ((j + 1) & 1)
static inline void bind_tick(soccer_handle* h, KernelParams& P, uint64_t ticks) {
    P.tick_in = h->d_tick + (h->tick_slot ? 16 : 0);
    P.tick_out = h->d_tick + (h->tick_slot ? 0 : 16);
    h->tick_slot ^= 1;
    if (h->capturing) { h->capture_ticks += ticks; h->capture_calls += 1; }
    else h->tick += ticks;
}

// soccer_graph_info's kernel_nodes: called next to every kernel launch of batched_step* / batched_rollout* / batched_reset
static inline void note_kernel(soccer_handle* h) { if (h->capturing) h->capture_kernels += 1; }

static inline int grid_for(const soccer_handle* h, uint64_t work_items) {
    uint64_t blocks = (work_items + kBlock - 1) / kBlock;
    if (blocks < 1) blocks = 1;
    if (blocks > (uint64_t)h->grid_cap) blocks = h->grid_cap;
    return static_cast<int>(blocks);
}

// ---- what one unit needs from another ------------------------------------------------------------
// soccer_rollout.hip: lets rollout_kernel<E, slip, lut_lds, *> of this handle's shape take `bytes` of dynamic LDS (soccer_create)
hipError_t rollout_raise_smem_limit(const soccer_handle* h, size_t bytes);
// soccer_rollout.hip: batched_rollout_ex behind its argument checks, counting episodes into `hist` (a captured run: flush_run)
int rollout_enqueue(soccer_handle* h, const soccer_rollout_args* a, const soccer_rollout_extra* x, unsigned long long* hist);
// soccer_step.hip: records the pending run of captured steps: one step as batched_step_ex would have, more as one rollout
int flush_run(soccer_handle* h);
// what every entry point that may put work on the stream during a capture calls first, so that the order of the calls is kept
static inline int flush_pending(soccer_handle* h) { return h->run.len ? flush_run(h) : SOCCER_OK; }
// soccer_comm.hip: destroys the handle's communicator, if it has one (the handle's destructor)
void comm_release(soccer_handle* h);
// soccer_learners.hip: frees the learners the caller did not destroy (the handle's destructor; the stream has drained)
void learners_release(soccer_handle* h);
// soccer_pairs.hip: frees the gradient-play learners the caller did not destroy (the handle's destructor; the stream has drained)
void gradient_players_release(soccer_handle* h);
// soccer_planners.hip and soccer_pairs.hip: sweeps a two-player solver enqueues between two synchronisations
constexpr int kMinimaxBatch = 16;
// soccer_planners.hip: the checks every two-player solver begins with: the handle, no capture, no fixed policy, gamma in [0, 1]
int minimax_check(soccer_handle* h, const char* what, double gamma);
// soccer_planners.hip: after every argument is checked: the device and the cached two-player lists (h->mm)
int minimax_prepare(soccer_handle* h);
// soccer_planners.hip: soccer_minimax_q_create's check of opponent_policy, on every live row of n policies (row 0 is not read)
int response_rows(soccer_handle* h, const char* what, const char* name, int n, const double* pol);
// soccer_planners.hip: n policies into a device block, row 0 of each as zeros
int response_upload(soccer_handle* h, double* dst, const double* pol, int n, hipMemcpyKind kind = hipMemcpyHostToDevice);

#pragma GCC visibility pop
