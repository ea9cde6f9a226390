// soccer_learners.hip — the nine kinds of learners (see soccer_handle.hpp): the minimax-Q learner soccer_minimax_q_*, the
// independent Q-learners soccer_q_learner_*, the policy hill-climbers soccer_wolf_phc_*, the regret matchers
// soccer_regret_learner_*, and the populations of one-actor learners, a member per lane: soccer_q_population_*,
// soccer_wolf_population_*, soccer_minimax_q_population_*, soccer_om_population_*, soccer_regret_population_*.
//
// What the kinds share comes first and is written once: the registry of live learners with its checks and destroy, the
// kernel-shape dispatch, the prologue and the hyperparameter checks of a creation, the messages of a refused table
// (soccer_policy_rows.hpp finds the place), the run loops, and the staged row mover of the populations.  A kind then
// brings its struct, its kernels' launches and its entry points, each a function of its own under its own name.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "soccer_dispatch.hpp"
#include "soccer_handle.hpp"
#include "soccer_learner_kernels.hpp"
#include "soccer_policy_rows.hpp"

// =================================================================================================
// the registry: one list of live learners in the handle, one check, one destroy
// =================================================================================================
// an environment variable of the tests, read at creation: its value if it is in lo .. hi, else `otherwise`
static long env_in(const char* name, long lo, long hi, long otherwise) {
    if (const char* e = std::getenv(name)) {
        const long v = std::atol(e);
        if (v >= lo && v <= hi) return v;
    }
    return otherwise;
}

// A learner: its device memory (one owner, like every other block of the library); a kind adds the argument block of its
// kernels.  The handle lists the live ones and frees what is left when it goes.
#pragma GCC visibility push(hidden)      // (their vtables are no exports of the library)
struct Learner {
    soccer_handle* const h;
    const int kind;                     // T::kKind of the struct this is
    OwnedBufs bufs;
    Learner(soccer_handle* handle, int k, const char* owner) : h(handle), kind(k), bufs(owner) {}
    virtual ~Learner() = default;
};

// a population, a member per lane: alpha lives per member in device memory, no slots
struct Population : Learner {
    static constexpr const char* kNoun = "population";
    const unsigned long long n;         // members = the handle's lanes
    const int launch_steps;             // steps per run kernel launch (SOCCER_POP_LAUNCH_STEPS, tests: a launch boundary within a short run)
    Population(soccer_handle* handle, int k, const char* owner)
        : Learner(handle, k, owner), n(handle->cfg.n_lanes), launch_steps((int)env_in("SOCCER_POP_LAUNCH_STEPS", 1, 4096, 4096)) {}
};

struct soccer_minimax_q : Learner {
    static constexpr int kKind = 0;
    static constexpr const char* kNoun = "learner";
    LearnerIO io{};
    int slot = 0;                       // alpha slot the NEXT update reads
    explicit soccer_minimax_q(soccer_handle* handle) : Learner(handle, kKind, "the minimax-Q learner") {}
};

struct soccer_q_learner : Learner {
    static constexpr int kKind = 1;
    static constexpr const char* kNoun = "learner";
    QLearnerIO io{};
    int slot = 0;                       // alpha slot the NEXT update reads
    explicit soccer_q_learner(soccer_handle* handle) : Learner(handle, kKind, "the Q-learner") {}
};

struct soccer_wolf_phc : Learner {
    static constexpr int kKind = 2;
    static constexpr const char* kNoun = "learner";
    PhcIO io{};
    int slot = 0;                       // alpha / dscale slot the NEXT update reads
    explicit soccer_wolf_phc(soccer_handle* handle) : Learner(handle, kKind, "the WoLF-PHC learner") {}
};

struct soccer_q_population : Population {
    static constexpr int kKind = 3;
    PopIO io{};
    int grid_blocks = 0;                // workgroups per run / update launch at most (SOCCER_POP_GRID_BLOCKS); 0: the handle's cap alone
    PopLeagueIO league{};               // K == 0: no league; else pop_league_run_kernel runs it
    explicit soccer_q_population(soccer_handle* handle) : Population(handle, kKind, "the population of Q-learners") {}
};

// alpha and dscale live per member in device memory
struct soccer_wolf_population : Population {
    static constexpr int kKind = 4;
    PhcPopIO io{};
    int grid_blocks = 0;                // as soccer_q_population's
    explicit soccer_wolf_population(soccer_handle* handle) : Population(handle, kKind, "the population of WoLF-PHC learners") {}
};

// a member is a wave of mq_pop_run_kernel
struct soccer_minimax_q_population : Population {
    static constexpr int kKind = 5;
    MqPopIO io{};
    unsigned waves = 1;                 // workgroups (of one wave) per launch at most: one episode-histogram slot each
    explicit soccer_minimax_q_population(soccer_handle* handle) : Population(handle, kKind, "the population of minimax-Q learners") {}
};

// a member is a thread of om_pop_run_kernel; io.Q is the members' rows [n][nS][kOmRow]
struct soccer_om_population : Population {
    static constexpr int kKind = 6;
    PopIO io{};
    int grid_blocks = 0;                // as soccer_q_population's
    explicit soccer_om_population(soccer_handle* handle) : Population(handle, kKind, "the population of opponent-modelling Q-learners") {}
};

// a member is a thread of rm_pop_run_kernel; a FIXED player's rows are a buffer of their own
struct soccer_regret_population : Population {
    static constexpr int kKind = 7;
    RmPopIO io{};
    int grid_blocks = 0;                // as soccer_q_population's
    explicit soccer_regret_population(soccer_handle* handle) : Population(handle, kKind, "the population of regret matchers") {}
};

// the regret matchers of one table: a FIXED player's rows are a buffer of their own (its Vq needs them)
struct soccer_regret_learner : Learner {
    static constexpr int kKind = 8;
    static constexpr const char* kNoun = "learner";
    RmIO io{};
    int slot = 0;                       // alpha slot the NEXT update reads
    explicit soccer_regret_learner(soccer_handle* handle) : Learner(handle, kKind, "the regret-matching learner") {}
};
#pragma GCC visibility pop

void learners_release(soccer_handle* h) {
    for (Learner* q : h->learners) delete q;
    h->learners.clear();
}

// What every entry point checks first.  The caller's pointer is only COMPARED with the handle's list, never read: a
// destroyed learner or one of another handle is refused untouched, and the kind is read from the list's own live entry.
static int learner_check(soccer_handle* h, const Learner* q, int kind, const char* noun, const char* what) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "%s during graph capture", what);
    const auto it = q ? std::find(h->learners.begin(), h->learners.end(), q) : h->learners.end();
    if (it == h->learners.end() || (*it)->kind != kind) return fail(h, SOCCER_E_INVALID, "%s: not a %s of this handle", what, noun);
    return SOCCER_OK;
}

template <class T>
static int check(soccer_handle* h, T* q, const char* what) {
    return learner_check(h, static_cast<const Learner*>(q), T::kKind, T::kNoun, what);
}

template <class T>
static int destroy(soccer_handle* h, T* q, const char* what) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (!q) return SOCCER_OK;
    if (int rc = check(h, q, what)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // nothing is freed under a kernel that reads it
    h->learners.erase(std::find(h->learners.begin(), h->learners.end(), static_cast<Learner*>(q)));
    delete q;
    return SOCCER_OK;
}

static int range_check(soccer_handle* h, const Population* q, const char* what, int64_t first, int64_t count) {
    if (first < 0 || count < 0 || (uint64_t)first > q->n || (uint64_t)count > q->n - (uint64_t)first)
        return fail(h, SOCCER_E_INVALID, "%s: members %lld .. %lld + %lld are outside the population of %llu", what, (long long)first,
                    (long long)first, (long long)count, q->n);
    return SOCCER_OK;
}

// what *_run checks before its first launch
template <class T>
static int run_check(soccer_handle* h, T* q, int32_t n_steps, const char* what) {
    if (int rc = check(h, q, what)) return rc;
    if (n_steps < 0) return fail(h, SOCCER_E_INVALID, "%s: n_steps must be >= 0", what);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return SOCCER_OK;
}

// the six arrays of *_update
static int transitions_check(soccer_handle* h, const char* what, bool required, const uint16_t* obs, const int8_t* act_a, const int8_t* act_b,
                             const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs) {
    if (required && (!obs || !act_a || !act_b || !reward || !terminated || !next_obs))
        return fail(h, SOCCER_E_INVALID, "%s: all six transition arrays are required", what);
    if (!aligned(obs, 2) || !aligned(next_obs, 2)) return fail(h, SOCCER_E_INVALID, "%s: obs / next_obs must be 2-byte aligned", what);
    return SOCCER_OK;
}

// =================================================================================================
// creation
// =================================================================================================
// what every creation checks first
template <class T>
static int create_check(soccer_handle* h, const void* cfg, T** out, const char* what) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "%s during graph capture", what);
    if (!cfg || !out) return fail(h, SOCCER_E_INVALID, "%s: cfg/out is NULL", what);
    *out = nullptr;
    if (h->P.policy_a != nullptr || h->P.policy_b != nullptr)
        return fail(h, SOCCER_E_INVALID, "%s needs a two-player handle: neither side may have a fixed policy (soccer_set_policy)", what);
    if (!(h->cfg.flags & SOCCER_F_AUTORESET)) return fail(h, SOCCER_E_INVALID, "%s needs a handle created with SOCCER_F_AUTORESET", what);
    return SOCCER_OK;
}

// ... and what it does last: it waits for its copies and launches (the vectors and the caller's arrays they read are
// pageable host memory of this call), then the handle lists the learner and the caller gets it
template <class T>
static int created(std::unique_ptr<T>& owner, T** out) {
    soccer_handle* const h = owner->h;
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->learners.push_back(owner.get());
    *out = owner.release();
    return SOCCER_OK;
}

static bool in_unit(double x) { return x >= 0.0 && x <= 1.0; }        // [0, 1]
static bool in_factor(double x) { return x > 0.0 && x <= 1.0; }       // (0, 1]
static bool in_discount(double x) { return x >= 0.0 && x < 1.0; }     // [0, 1)
static bool in_q(double x) { return x >= -1.0 && x <= 1.0; }          // [-1, 1]

// the three single learners: the lane limit of their integer sums, and the five scalars of every config
template <class Cfg>
static int single_check(soccer_handle* h, const Cfg* cfg, const char* what) {
    if (h->cfg.n_lanes > SOCCER_MQ_MAX_LANES)
        return fail(h, SOCCER_E_INVALID, "%s: more than 2^22 lanes (%llu): the integer sums of a step could overflow", what,
                    (unsigned long long)h->cfg.n_lanes);
    if (!in_discount(cfg->discount_factor)) return fail(h, SOCCER_E_INVALID, "discount_factor must be in [0, 1)");
    if (!in_unit(cfg->alpha)) return fail(h, SOCCER_E_INVALID, "alpha must be in [0, 1]");
    if (!in_factor(cfg->decay)) return fail(h, SOCCER_E_INVALID, "decay must be in (0, 1]");
    if (!in_unit(cfg->explor)) return fail(h, SOCCER_E_INVALID, "explor must be in [0, 1]");
    if (!in_q(cfg->q_init)) return fail(h, SOCCER_E_INVALID, "q_init must be in [-1, 1]");
    return SOCCER_OK;
}

// a hyperparameter of every member: the caller's n values, each held to the scalar's range, or the scalar n times
static int pop_param(soccer_handle* h, const char* name, const char* range, const double* per_member, double scalar, size_t n,
                     bool (*ok)(double), std::vector<double>& out) {
    if (!per_member) {
        if (!ok(scalar)) return fail(h, SOCCER_E_INVALID, "%s must be in %s", name, range);
        out.assign(n, scalar);
        return SOCCER_OK;
    }
    for (size_t i = 0; i < n; ++i)
        if (!ok(per_member[i])) return fail(h, SOCCER_E_INVALID, "%s_per_member[%zu] must be in %s", name, i, range);
    out.assign(per_member, per_member + n);
    return SOCCER_OK;
}

// the three populations: par[0 .. 3] = alpha, decay, explor, discount_factor of every member, and q_init
template <class Cfg>
static int pop_params(soccer_handle* h, const Cfg* cfg, size_t n, std::vector<double>* par) {
    if (int rc = pop_param(h, "discount_factor", "[0, 1)", cfg->discount_factor_per_member, cfg->discount_factor, n, in_discount, par[3])) return rc;
    if (int rc = pop_param(h, "alpha", "[0, 1]", cfg->alpha_per_member, cfg->alpha, n, in_unit, par[0])) return rc;
    if (int rc = pop_param(h, "decay", "(0, 1]", cfg->decay_per_member, cfg->decay, n, in_factor, par[1])) return rc;
    if (int rc = pop_param(h, "explor", "[0, 1]", cfg->explor_per_member, cfg->explor, n, in_unit, par[2])) return rc;
    if (!in_q(cfg->q_init)) return fail(h, SOCCER_E_INVALID, "q_init must be in [-1, 1]");
    return SOCCER_OK;
}

// =================================================================================================
// the messages of a refused table; soccer_policy_rows.hpp finds the place
// =================================================================================================
// `what` NULL: no entry point's name in front; members: the place has a member index
static int rows_fail(soccer_handle* h, const char* what, const char* name, bool members, const RowFault& f) {
    char at[192];
    int k = std::snprintf(at, sizeof at, "%s%s%s", what ? what : "", what ? ": " : "", name);
    if (members) std::snprintf(at + k, sizeof at - (size_t)k, "[%zu]", f.member);
    if (f.action == 5) return fail(h, SOCCER_E_INVALID, "%s[%d] does not sum to 1", at, f.state);
    return fail(h, SOCCER_E_INVALID, "%s[%d][%d] is negative or not a number", at, f.state, f.action);
}

// rows first_row.. of `members` policies [nS][5] each, held to what thresholds holds a fixed policy to
static int rows_check(soccer_handle* h, const char* what, const char* name, const double* policy, size_t members, int nS, int first_row) {
    RowFault f;
    return policy_rows_check(policy, members, nS, first_row, &f) ? SOCCER_OK : rows_fail(h, what, name, true, f);
}

// a fixed mixed policy's threshold rows [nS][4], appended to `rows`
static int thresholds(soccer_handle* h, const char* name, const double* policy, int nS, std::vector<uint16_t>& rows) {
    RowFault f;
    const size_t at = rows.size();
    rows.resize(at + (size_t)nS * 4);
    return fixed_thresholds(policy, nS, rows.data() + at, &f) ? SOCCER_OK : rows_fail(h, nullptr, name, false, f);
}

// `members` tables [nS][width] of a checkpoint in [-1, 1] (members 0: one table, and no member index in the message);
// width 25: a joint-action table, whose last index is two
static int bounds_check(soccer_handle* h, const char* what, const char* name, const double* q, size_t members, size_t nS, size_t width) {
    const size_t i = q_bounds_check(q, std::max<size_t>(members, 1), nS, width);
    if (i == kInBounds) return SOCCER_OK;
    char at[96];
    int k = members ? std::snprintf(at, sizeof at, "[%zu]", i / width / nS) : 0;
    k += std::snprintf(at + k, sizeof at - (size_t)k, "[%zu]", i / width % nS);
    if (width == 25) k += std::snprintf(at + k, sizeof at - (size_t)k, "[%zu]", i % 25 / 5);
    if (width > 1) std::snprintf(at + k, sizeof at - (size_t)k, "[%zu]", i % 5);
    return fail(h, SOCCER_E_INVALID, "%s: %s%s is outside [-1, 1]", what, name, at);
}

// `count` values of a checkpoint in [0, 1] (alpha, dscale)
static int unit_check(soccer_handle* h, const char* what, const char* name, const double* v, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (!in_unit(v[i])) return fail(h, SOCCER_E_INVALID, "%s: %s[%zu] must be in [0, 1]", what, name, i);
    return SOCCER_OK;
}

// =================================================================================================
// the single learners: a step is an act kernel and an update kernel
// =================================================================================================
// the act kernel of the learner whose argument block this is
template <class IO>
static hipError_t act(soccer_handle* h, const KernelParams& P, const IO& io) {
    return with_shape(h, [&](auto slip, auto lds) {
        const dim3 grid(grid_for(h, P.n)), block(kBlock);
        if constexpr (std::is_same_v<IO, LearnerIO>) hipLaunchKernelGGL((learner_act_kernel<slip, lds>), grid, block, h->smem_bytes, h->stream, P, io);
        else if constexpr (std::is_same_v<IO, QLearnerIO>) hipLaunchKernelGGL((q_act_kernel<slip, lds>), grid, block, h->smem_bytes, h->stream, P, io);
        else if constexpr (std::is_same_v<IO, PhcIO>) hipLaunchKernelGGL((phc_act_kernel<slip, lds>), grid, block, h->smem_bytes, h->stream, P, io);
        else hipLaunchKernelGGL((rm_act_kernel<slip, lds>), grid, block, h->smem_bytes, h->stream, P, io);
        return hipSuccess;
    });
}

static unsigned mq_update_grid(int nS) { return (unsigned)((nS + kLearnerWaves - 1) / kLearnerWaves); }
static unsigned q_update_grid(int nS) { return (unsigned)((nS + kQStates - 1) / kQStates); }

// ... and its update kernel, which reads the alpha slot the last one wrote
template <class T>
static void launch_update(T* q) {
    const dim3 block(kLearnerBlock);
    if constexpr (std::is_same_v<T, soccer_minimax_q>) hipLaunchKernelGGL(learner_update_kernel<0>, dim3(mq_update_grid(q->io.nS)), block, 0, q->h->stream, q->io, q->slot);
    else if constexpr (std::is_same_v<T, soccer_q_learner>) hipLaunchKernelGGL(q_update_kernel<0>, dim3(q_update_grid(q->io.nS)), block, 0, q->h->stream, q->io, q->slot);
    else if constexpr (std::is_same_v<T, soccer_wolf_phc>) hipLaunchKernelGGL(phc_update_kernel<0>, dim3(q_update_grid(q->io.nS)), block, 0, q->h->stream, q->io, q->slot);
    else hipLaunchKernelGGL(rm_update_kernel<0>, dim3(q_update_grid(q->io.nS)), block, 0, q->h->stream, q->io, q->slot);
    q->slot ^= 1;
}

template <class T>
static int learner_run(soccer_handle* h, T* q, int32_t n_steps, const char* what) {
    if (int rc = run_check(h, q, n_steps, what)) return rc;
    for (int32_t t = 0; t < n_steps; ++t) {
        KernelParams P = h->P;
        bind_tick(h, P, 1);
        HIP_TRY(h, act(h, P, q->io));
        launch_update(q);
    }
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

// what *_update of a single learner checks before its launches
template <class T>
static int learner_update_check(soccer_handle* h, T* q, const char* what, int64_t n, const uint16_t* obs, const int8_t* act_a, const int8_t* act_b,
                                const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs) {
    if (int rc = check(h, q, what)) return rc;
    if (n < 0 || n > (int64_t)SOCCER_MQ_MAX_LANES) return fail(h, SOCCER_E_INVALID, "%s: n must be in 0..2^22", what);
    if (int rc = transitions_check(h, what, n > 0, obs, act_a, act_b, reward, terminated, next_obs)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return SOCCER_OK;
}

// ---- the minimax-Q learner: soccer_minimax_q_* ----------------------------------------------------
extern "C" int soccer_minimax_q_create(soccer_handle* h, const soccer_minimax_q_config* cfg, soccer_minimax_q** out) {
    if (int rc = create_check(h, cfg, out, "soccer_minimax_q_create")) return rc;
    if (int rc = single_check(h, cfg, "soccer_minimax_q_create")) return rc;
    if (cfg->opponent != SOCCER_MQ_UNIFORM && cfg->opponent != SOCCER_MQ_SELF && cfg->opponent != SOCCER_MQ_FIXED)
        return fail(h, SOCCER_E_INVALID, "opponent must be SOCCER_MQ_UNIFORM, SOCCER_MQ_SELF or SOCCER_MQ_FIXED");
    if ((cfg->opponent == SOCCER_MQ_FIXED) != (cfg->opponent_policy != nullptr))
        return fail(h, SOCCER_E_INVALID, "opponent_policy goes with SOCCER_MQ_FIXED, and only with it");
    const int nS = h->rules.nS;
    std::vector<uint16_t> fixed;
    if (cfg->opponent == SOCCER_MQ_FIXED)
        if (int rc = thresholds(h, "opponent_policy", cfg->opponent_policy, nS, fixed)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, with_shape(h, [&](auto slip, auto lds) { return raise_lds_limit(h, learner_act_kernel<slip, lds>); }));
    std::unique_ptr<soccer_minimax_q> owner(new soccer_minimax_q(h));
    soccer_minimax_q* q = owner.get();
    LearnerIO& io = q->io;
    const size_t cells = (size_t)nS * 25;
    int rc = q->bufs.alloc(h, cells, &io.Q);
    if (!rc) rc = q->bufs.alloc(h, (size_t)nS, &io.V);
    if (!rc) rc = q->bufs.alloc(h, (size_t)nS * 5, &io.pi_a);
    if (!rc) rc = q->bufs.alloc(h, (size_t)nS * 5, &io.pi_b);
    if (!rc) rc = q->bufs.alloc(h, (size_t)nS, &io.Vq);
    if (!rc) rc = q->bufs.alloc(h, cells, &io.visits);
    if (!rc) rc = q->bufs.alloc(h, cells, &io.cnt);
    if (!rc) rc = q->bufs.alloc(h, cells, &io.rsum);
    if (!rc) rc = q->bufs.alloc(h, cells, &io.sv);
    if (!rc) rc = q->bufs.alloc(h, (size_t)nS * 4, &io.mix_a);
    if (!rc && cfg->opponent != SOCCER_MQ_UNIFORM) rc = q->bufs.alloc(h, (size_t)nS * 4, &io.mix_b);
    if (!rc) rc = q->bufs.alloc(h, 2, &io.alpha);
    if (!rc) rc = q->bufs.alloc(h, 1, &io.steps);
    if (rc) return rc;
    io.misuse = h->d_misuse;
    io.gamma = cfg->discount_factor; io.decay = cfg->decay; io.explor = cfg->explor;
    io.nS = nS; io.self_play = cfg->opponent == SOCCER_MQ_SELF ? 1 : 0;
    if (cfg->opponent == SOCCER_MQ_FIXED)
        HIP_TRY(h, hipMemcpyAsync(io.mix_b, fixed.data(), fixed.size() * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(learner_init_kernel, dim3((unsigned)((cells + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, io, cfg->q_init, cfg->alpha);
    return created(owner, out);
}

extern "C" int soccer_minimax_q_destroy(soccer_handle* h, soccer_minimax_q* q) { return destroy(h, q, "soccer_minimax_q_destroy"); }

extern "C" int soccer_minimax_q_run(soccer_handle* h, soccer_minimax_q* q, int32_t n_steps) {
    return learner_run(h, q, n_steps, "soccer_minimax_q_run");
}

extern "C" int soccer_minimax_q_update(soccer_handle* h, soccer_minimax_q* q, int64_t n, const uint16_t* obs, const int8_t* act_a,
                                       const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs) {
    if (int rc = learner_update_check(h, q, "soccer_minimax_q_update", n, obs, act_a, act_b, reward, terminated, next_obs)) return rc;
    if (n > 0)
        hipLaunchKernelGGL(learner_reduce_kernel, dim3(grid_for(h, (uint64_t)n)), dim3(kBlock), 0, h->stream, q->io, (long long)n,
                           obs, act_a, act_b, reward, terminated, next_obs);
    launch_update(q);
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

extern "C" int soccer_minimax_q_read(soccer_handle* h, soccer_minimax_q* q, double* Q, double* V, double* pi_a, double* pi_b,
                                     uint64_t* visits, double* alpha, uint64_t* steps) {
    if (int rc = check(h, q, "soccer_minimax_q_read")) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const LearnerIO& io = q->io;
    const size_t nS = (size_t)io.nS;
    if (Q) HIP_TRY(h, hipMemcpyAsync(Q, io.Q, nS * 200, hipMemcpyDeviceToHost, h->stream));
    if (V) HIP_TRY(h, hipMemcpyAsync(V, io.V, nS * 8, hipMemcpyDeviceToHost, h->stream));
    if (pi_a) HIP_TRY(h, hipMemcpyAsync(pi_a, io.pi_a, nS * 40, hipMemcpyDeviceToHost, h->stream));
    if (pi_b) HIP_TRY(h, hipMemcpyAsync(pi_b, io.pi_b, nS * 40, hipMemcpyDeviceToHost, h->stream));
    if (visits) HIP_TRY(h, hipMemcpyAsync(visits, io.visits, nS * 200, hipMemcpyDeviceToHost, h->stream));
    if (alpha) HIP_TRY(h, hipMemcpyAsync(alpha, io.alpha + q->slot, 8, hipMemcpyDeviceToHost, h->stream));
    if (steps) HIP_TRY(h, hipMemcpyAsync(steps, io.steps, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SOCCER_OK;
}

extern "C" int soccer_minimax_q_load(soccer_handle* h, soccer_minimax_q* q, const double* Q, const uint64_t* visits,
                                     const double* alpha, const uint64_t* steps) {
    if (int rc = check(h, q, "soccer_minimax_q_load")) return rc;
    if (!Q) return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_load: Q is NULL");
    const LearnerIO& io = q->io;
    const size_t nS = (size_t)io.nS;
    if (int rc = bounds_check(h, "soccer_minimax_q_load", "Q", Q, 0, nS, 25)) return rc;
    if (alpha && !in_unit(*alpha)) return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_load: alpha must be in [0, 1]");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipMemsetAsync(io.Q, 0, 200, h->stream));                          // Q[0] = 0
    HIP_TRY(h, hipMemcpyAsync(io.Q + 25, Q + 25, (nS - 1) * 200, hipMemcpyHostToDevice, h->stream));
    if (visits) HIP_TRY(h, hipMemcpyAsync(io.visits, visits, nS * 200, hipMemcpyHostToDevice, h->stream));
    if (alpha) HIP_TRY(h, hipMemcpyAsync(io.alpha + q->slot, alpha, 8, hipMemcpyHostToDevice, h->stream));
    if (steps) HIP_TRY(h, hipMemcpyAsync(io.steps, steps, 8, hipMemcpyHostToDevice, h->stream));
    const unsigned grid = mq_update_grid(io.nS);
    if (visits) hipLaunchKernelGGL(learner_update_kernel<1>, dim3(grid),dim3(kLearnerBlock), 0, h->stream, io, q->slot);
    else hipLaunchKernelGGL(learner_update_kernel<2>, dim3(grid), dim3(kLearnerBlock), 0, h->stream, io, q->slot);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // the caller's arrays are pageable host memory
    return SOCCER_OK;
}

// ---- independent Q-learners: soccer_q_learner_* ---------------------------------------------------
static bool ql_kind(int32_t k) { return k == SOCCER_QL_GREEDY || k == SOCCER_QL_UNIFORM || k == SOCCER_QL_FIXED; }

extern "C" int soccer_q_learner_create(soccer_handle* h, const soccer_q_learner_config* cfg, soccer_q_learner** out) {
    if (int rc = create_check(h, cfg, out, "soccer_q_learner_create")) return rc;
    if (int rc = single_check(h, cfg, "soccer_q_learner_create")) return rc;
    if (!ql_kind(cfg->act_a) || !ql_kind(cfg->act_b))
        return fail(h, SOCCER_E_INVALID, "act_a / act_b must be SOCCER_QL_GREEDY, SOCCER_QL_UNIFORM or SOCCER_QL_FIXED");
    if ((cfg->act_a == SOCCER_QL_FIXED) != (cfg->policy_a != nullptr)) return fail(h, SOCCER_E_INVALID, "policy_a goes with act_a == SOCCER_QL_FIXED, and only with it");
    if ((cfg->act_b == SOCCER_QL_FIXED) != (cfg->policy_b != nullptr)) return fail(h, SOCCER_E_INVALID, "policy_b goes with act_b == SOCCER_QL_FIXED, and only with it");
    const int nS = h->rules.nS;
    std::vector<uint16_t> fixed[2];
    if (cfg->policy_a) if (int rc = thresholds(h, "policy_a", cfg->policy_a, nS, fixed[0])) return rc;
    if (cfg->policy_b) if (int rc = thresholds(h, "policy_b", cfg->policy_b, nS, fixed[1])) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, with_shape(h, [&](auto slip, auto lds) { return raise_lds_limit(h, q_act_kernel<slip, lds>); }));
    std::unique_ptr<soccer_q_learner> owner(new soccer_q_learner(h));
    soccer_q_learner* q = owner.get();
    QLearnerIO& io = q->io;
    const size_t cells = (size_t)nS * 25;
    int rc = SOCCER_OK;
    for (int p = 0; p < 2; ++p) {
        if (!rc) rc = q->bufs.alloc(h, (size_t)nS * 5, &io.Q[p]);
        if (!rc) rc = q->bufs.alloc(h, (size_t)nS, &io.Vq[p]);
        if (!rc) rc = q->bufs.alloc(h, cells, &io.sv[p]);
    }
    if (!rc) rc = q->bufs.alloc(h, cells, &io.visits);
    if (!rc) rc = q->bufs.alloc(h, cells, &io.cnt);
    if (!rc) rc = q->bufs.alloc(h, cells, &io.rsum);
    if (!rc && cfg->act_a != SOCCER_QL_UNIFORM) rc = q->bufs.alloc(h, (size_t)nS * 4, &io.mix_a);
    if (!rc && cfg->act_b != SOCCER_QL_UNIFORM) rc = q->bufs.alloc(h, (size_t)nS * 4, &io.mix_b);
    if (!rc) rc = q->bufs.alloc(h, 2, &io.alpha);
    if (!rc) rc = q->bufs.alloc(h, 1, &io.steps);
    if (rc) return rc;
    io.misuse = h->d_misuse;
    io.gamma = cfg->discount_factor; io.decay = cfg->decay; io.explor = cfg->explor;
    io.nS = nS;
    io.greedy[0] = cfg->act_a == SOCCER_QL_GREEDY ? 1 : 0; io.greedy[1] = cfg->act_b == SOCCER_QL_GREEDY ? 1 : 0;
    if (cfg->policy_a) HIP_TRY(h, hipMemcpyAsync(io.mix_a, fixed[0].data(), fixed[0].size() * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
    if (cfg->policy_b) HIP_TRY(h, hipMemcpyAsync(io.mix_b, fixed[1].data(), fixed[1].size() * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(q_init_kernel, dim3((unsigned)((cells + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, io, cfg->q_init, cfg->alpha);
    hipLaunchKernelGGL(q_update_kernel<1>, dim3(q_update_grid(nS)), dim3(kLearnerBlock), 0, h->stream, io, 0);
    return created(owner, out);
}

extern "C" int soccer_q_learner_destroy(soccer_handle* h, soccer_q_learner* q) { return destroy(h, q, "soccer_q_learner_destroy"); }

extern "C" int soccer_q_learner_run(soccer_handle* h, soccer_q_learner* q, int32_t n_steps) {
    return learner_run(h, q, n_steps, "soccer_q_learner_run");
}

extern "C" int soccer_q_learner_update(soccer_handle* h, soccer_q_learner* q, int64_t n, const uint16_t* obs, const int8_t* act_a,
                                       const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs) {
    if (int rc = learner_update_check(h, q, "soccer_q_learner_update", n, obs, act_a, act_b, reward, terminated, next_obs)) return rc;
    if (n > 0)
        hipLaunchKernelGGL(q_reduce_kernel, dim3(grid_for(h, (uint64_t)n)), dim3(kBlock), 0, h->stream, q->io, (long long)n,
                           obs, act_a, act_b, reward, terminated, next_obs);
    launch_update(q);
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

extern "C" int soccer_q_learner_read(soccer_handle* h, soccer_q_learner* q, double* Q_a, double* Q_b, uint64_t* visits,
                                     double* alpha, uint64_t* steps) {
    if (int rc = check(h, q, "soccer_q_learner_read")) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const QLearnerIO& io = q->io;
    const size_t nS = (size_t)io.nS;
    if (Q_a) HIP_TRY(h, hipMemcpyAsync(Q_a, io.Q[0], nS * 40, hipMemcpyDeviceToHost, h->stream));
    if (Q_b) HIP_TRY(h, hipMemcpyAsync(Q_b, io.Q[1], nS * 40, hipMemcpyDeviceToHost, h->stream));
    if (visits) HIP_TRY(h, hipMemcpyAsync(visits, io.visits, nS * 200, hipMemcpyDeviceToHost, h->stream));
    if (alpha) HIP_TRY(h, hipMemcpyAsync(alpha, io.alpha + q->slot, 8, hipMemcpyDeviceToHost, h->stream));
    if (steps) HIP_TRY(h, hipMemcpyAsync(steps, io.steps, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SOCCER_OK;
}

extern "C" int soccer_q_learner_load(soccer_handle* h, soccer_q_learner* q, const double* Q_a, const double* Q_b, const uint64_t* visits,
                                     const double* alpha, const uint64_t* steps) {
    if (int rc = check(h, q, "soccer_q_learner_load")) return rc;
    if (!Q_a || !Q_b) return fail(h, SOCCER_E_INVALID, "soccer_q_learner_load: Q_a / Q_b is NULL");
    const QLearnerIO& io = q->io;
    const size_t nS = (size_t)io.nS;
    const double* const Q[2] = {Q_a, Q_b};
    for (int p = 0; p < 2; ++p)
        if (int rc = bounds_check(h, "soccer_q_learner_load", p ? "Q_b" : "Q_a", Q[p], 0, nS, 5)) return rc;
    if (alpha && !in_unit(*alpha)) return fail(h, SOCCER_E_INVALID, "soccer_q_learner_load: alpha must be in [0, 1]");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    for (int p = 0; p < 2; ++p) {
        HIP_TRY(h, hipMemsetAsync(io.Q[p], 0, 40, h->stream));                    // Q_p[0] = 0
        HIP_TRY(h, hipMemcpyAsync(io.Q[p] + 5, Q[p] + 5, (nS - 1) * 40, hipMemcpyHostToDevice, h->stream));
    }
    if (visits) HIP_TRY(h, hipMemcpyAsync(io.visits, visits, nS * 200, hipMemcpyHostToDevice, h->stream));
    else HIP_TRY(h, hipMemsetAsync(io.visits, 0, nS * 200, h->stream));
    if (alpha) HIP_TRY(h, hipMemcpyAsync(io.alpha + q->slot, alpha, 8, hipMemcpyHostToDevice, h->stream));
    if (steps) HIP_TRY(h, hipMemcpyAsync(io.steps, steps, 8, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(q_update_kernel<1>, dim3(q_update_grid(io.nS)), dim3(kLearnerBlock), 0, h->stream, io, q->slot);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // the caller's arrays are pageable host memory
    return SOCCER_OK;
}

// ---- policy hill-climbers: soccer_wolf_phc_* ------------------------------------------------------
static bool phc_kind(int32_t k) { return k == SOCCER_PHC_LEARN || k == SOCCER_PHC_UNIFORM || k == SOCCER_PHC_FIXED; }

extern "C" int soccer_wolf_phc_create(soccer_handle* h, const soccer_wolf_phc_config* cfg, soccer_wolf_phc** out) {
    if (int rc = create_check(h, cfg, out, "soccer_wolf_phc_create")) return rc;
    if (int rc = single_check(h, cfg, "soccer_wolf_phc_create")) return rc;
    if (!in_unit(cfg->delta_win)) return fail(h, SOCCER_E_INVALID, "delta_win must be in [0, 1]");
    if (!in_unit(cfg->delta_lose)) return fail(h, SOCCER_E_INVALID, "delta_lose must be in [0, 1]");
    if (!in_factor(cfg->delta_decay)) return fail(h, SOCCER_E_INVALID, "delta_decay must be in (0, 1]");
    if (!phc_kind(cfg->act_a) || !phc_kind(cfg->act_b))
        return fail(h, SOCCER_E_INVALID, "act_a / act_b must be SOCCER_PHC_LEARN, SOCCER_PHC_UNIFORM or SOCCER_PHC_FIXED");
    if ((cfg->act_a == SOCCER_PHC_FIXED) != (cfg->policy_a != nullptr)) return fail(h, SOCCER_E_INVALID, "policy_a goes with act_a == SOCCER_PHC_FIXED, and only with it");
    if ((cfg->act_b == SOCCER_PHC_FIXED) != (cfg->policy_b != nullptr)) return fail(h, SOCCER_E_INVALID, "policy_b goes with act_b == SOCCER_PHC_FIXED, and only with it");
    const int nS = h->rules.nS;
    const int32_t kinds[2] = {cfg->act_a, cfg->act_b};
    const double* policy[2] = {cfg->policy_a, cfg->policy_b};
    std::vector<uint16_t> fixed[2];
    if (cfg->policy_a) if (int rc = thresholds(h, "policy_a", cfg->policy_a, nS, fixed[0])) return rc;
    if (cfg->policy_b) if (int rc = thresholds(h, "policy_b", cfg->policy_b, nS, fixed[1])) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, with_shape(h, [&](auto slip, auto lds) { return raise_lds_limit(h, phc_act_kernel<slip, lds>); }));
    std::unique_ptr<soccer_wolf_phc> owner(new soccer_wolf_phc(h));
    soccer_wolf_phc* q = owner.get();
    PhcIO& io = q->io;
    const size_t cells = (size_t)nS * 25;
    int rc = SOCCER_OK;
    for (int p = 0; p < 2; ++p) {
        if (!rc) rc = q->bufs.alloc(h, (size_t)nS * 5, &io.Q[p]);
        if (!rc) rc = q->bufs.alloc(h, (size_t)nS * 5, &io.pi[p]);
        if (!rc) rc = q->bufs.alloc(h, (size_t)nS * 5, &io.avg[p]);
        if (!rc) rc = q->bufs.alloc(h, (size_t)nS, &io.Vq[p]);
        if (!rc) rc = q->bufs.alloc(h, cells, &io.sv[p]);
    }
    if (!rc) rc = q->bufs.alloc(h, cells, &io.visits);
    if (!rc) rc = q->bufs.alloc(h, (size_t)nS, &io.updates);
    if (!rc) rc = q->bufs.alloc(h, cells, &io.cnt);
    if (!rc) rc = q->bufs.alloc(h, cells, &io.rsum);
    if (!rc && cfg->act_a != SOCCER_PHC_UNIFORM) rc = q->bufs.alloc(h, (size_t)nS * 4, &io.mix_a);
    if (!rc && cfg->act_b != SOCCER_PHC_UNIFORM) rc = q->bufs.alloc(h, (size_t)nS * 4, &io.mix_b);
    if (!rc) rc = q->bufs.alloc(h, 2, &io.alpha);
    if (!rc) rc = q->bufs.alloc(h, 2, &io.dscale);
    if (!rc) rc = q->bufs.alloc(h, 1, &io.steps);
    if (rc) return rc;
    io.misuse = h->d_misuse;
    io.gamma = cfg->discount_factor; io.decay = cfg->decay; io.explor = cfg->explor;
    io.nS = nS;
    io.delta_win = cfg->delta_win; io.delta_lose = cfg->delta_lose; io.delta_decay = cfg->delta_decay;
    for (int p = 0; p < 2; ++p) io.learn[p] = kinds[p] == SOCCER_PHC_LEARN ? 1 : 0;
    hipLaunchKernelGGL(phc_init_kernel, dim3((unsigned)((cells + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, io, cfg->q_init, cfg->alpha);
    for (int p = 0; p < 2; ++p) {
        if (!policy[p]) continue;
        HIP_TRY(h, hipMemcpyAsync(p ? io.mix_b : io.mix_a, fixed[p].data(), fixed[p].size() * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(io.pi[p], policy[p], (size_t)nS * 40, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(io.avg[p], policy[p], (size_t)nS * 40, hipMemcpyHostToDevice, h->stream));
    }
    hipLaunchKernelGGL(phc_update_kernel<1>, dim3(q_update_grid(nS)), dim3(kLearnerBlock), 0, h->stream, io, 0);
    return created(owner, out);
}

extern "C" int soccer_wolf_phc_destroy(soccer_handle* h, soccer_wolf_phc* q) { return destroy(h, q, "soccer_wolf_phc_destroy"); }

extern "C" int soccer_wolf_phc_run(soccer_handle* h, soccer_wolf_phc* q, int32_t n_steps) {
    return learner_run(h, q, n_steps, "soccer_wolf_phc_run");
}

extern "C" int soccer_wolf_phc_update(soccer_handle* h, soccer_wolf_phc* q, int64_t n, const uint16_t* obs, const int8_t* act_a,
                                      const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs) {
    if (int rc = learner_update_check(h, q, "soccer_wolf_phc_update", n, obs, act_a, act_b, reward, terminated, next_obs)) return rc;
    if (n > 0)
        hipLaunchKernelGGL(phc_reduce_kernel, dim3(grid_for(h, (uint64_t)n)), dim3(kBlock), 0, h->stream, q->io, (long long)n,
                           obs, act_a, act_b, reward, terminated, next_obs);
    launch_update(q);
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

extern "C" int soccer_wolf_phc_read(soccer_handle* h, soccer_wolf_phc* q, const soccer_wolf_phc_state* out) {
    if (int rc = check(h, q, "soccer_wolf_phc_read")) return rc;
    if (!out) return fail(h, SOCCER_E_INVALID, "soccer_wolf_phc_read: out is NULL");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const PhcIO& io = q->io;
    const size_t nS = (size_t)io.nS;
    double* const rows[6] = {out->Q_a, out->Q_b, out->pi_a, out->pi_b, out->avg_a, out->avg_b};
    const double* const from[6] = {io.Q[0], io.Q[1], io.pi[0], io.pi[1], io.avg[0], io.avg[1]};
    for (int i = 0; i < 6; ++i)
        if (rows[i]) HIP_TRY(h, hipMemcpyAsync(rows[i], from[i], nS * 40, hipMemcpyDeviceToHost, h->stream));
    if (out->visits) HIP_TRY(h, hipMemcpyAsync(out->visits, io.visits, nS * 200, hipMemcpyDeviceToHost, h->stream));
    if (out->updates) HIP_TRY(h, hipMemcpyAsync(out->updates, io.updates, nS * 8, hipMemcpyDeviceToHost, h->stream));
    if (out->alpha) HIP_TRY(h, hipMemcpyAsync(out->alpha, io.alpha + q->slot, 8, hipMemcpyDeviceToHost, h->stream));
    if (out->dscale) HIP_TRY(h, hipMemcpyAsync(out->dscale, io.dscale + q->slot, 8, hipMemcpyDeviceToHost, h->stream));
    if (out->steps) HIP_TRY(h, hipMemcpyAsync(out->steps, io.steps, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SOCCER_OK;
}

extern "C" int soccer_wolf_phc_load(soccer_handle* h, soccer_wolf_phc* q, const soccer_wolf_phc_state* in) {
    if (int rc = check(h, q, "soccer_wolf_phc_load")) return rc;
    if (!in || !in->Q_a || !in->Q_b) return fail(h, SOCCER_E_INVALID, "soccer_wolf_phc_load: in / Q_a / Q_b is NULL");
    const PhcIO& io = q->io;
    const size_t nS = (size_t)io.nS;
    const double* const Q[2] = {in->Q_a, in->Q_b};
    // a player that does not LEARN keeps its constant rows
    const double* rows[4] = {io.learn[0] ? in->pi_a : nullptr, io.learn[1] ? in->pi_b : nullptr,
                             io.learn[0] ? in->avg_a : nullptr, io.learn[1] ? in->avg_b : nullptr};
    double* const to[4] = {io.pi[0], io.pi[1], io.avg[0], io.avg[1]};
    static const char* const names[4] = {"pi_a", "pi_b", "avg_a", "avg_b"};
    for (int p = 0; p < 2; ++p)
        if (int rc = bounds_check(h, "soccer_wolf_phc_load", p ? "Q_b" : "Q_a", Q[p], 0, nS, 5)) return rc;
    RowFault f;
    for (int i = 0; i < 4; ++i)
        if (rows[i] && !policy_rows_check(rows[i], 1, io.nS, 1, &f)) return rows_fail(h, "soccer_wolf_phc_load", names[i], false, f);
    if (in->alpha && !in_unit(*in->alpha)) return fail(h, SOCCER_E_INVALID, "soccer_wolf_phc_load: alpha must be in [0, 1]");
    if (in->dscale && !in_unit(*in->dscale)) return fail(h, SOCCER_E_INVALID, "soccer_wolf_phc_load: dscale must be in [0, 1]");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    for (int p = 0; p < 2; ++p) {
        HIP_TRY(h, hipMemsetAsync(io.Q[p], 0, 40, h->stream));                    // Q_p[0] = 0
        HIP_TRY(h, hipMemcpyAsync(io.Q[p] + 5, Q[p] + 5, (nS - 1) * 40, hipMemcpyHostToDevice, h->stream));
    }
    for (int i = 0; i < 4; ++i)                                                   // (row 0 stays what creation gave it)
        if (rows[i]) HIP_TRY(h, hipMemcpyAsync(to[i] + 5, rows[i] + 5, (nS - 1) * 40, hipMemcpyHostToDevice, h->stream));
    if (in->visits) HIP_TRY(h, hipMemcpyAsync(io.visits, in->visits, nS * 200, hipMemcpyHostToDevice, h->stream));
    else HIP_TRY(h, hipMemsetAsync(io.visits, 0, nS * 200, h->stream));
    if (in->updates) HIP_TRY(h, hipMemcpyAsync(io.updates, in->updates, nS * 8, hipMemcpyHostToDevice, h->stream));
    else HIP_TRY(h, hipMemsetAsync(io.updates, 0, nS * 8, h->stream));
    if (in->alpha) HIP_TRY(h, hipMemcpyAsync(io.alpha + q->slot, in->alpha, 8, hipMemcpyHostToDevice, h->stream));
    if (in->dscale) HIP_TRY(h, hipMemcpyAsync(io.dscale + q->slot, in->dscale, 8, hipMemcpyHostToDevice, h->stream));
    if (in->steps) HIP_TRY(h, hipMemcpyAsync(io.steps, in->steps, 8, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(phc_update_kernel<1>, dim3(q_update_grid(io.nS)), dim3(kLearnerBlock), 0, h->stream, io, q->slot);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // the caller's arrays are pageable host memory
    return SOCCER_OK;
}

// =================================================================================================
// the populations: a run is a few launches of many steps each, a member's row of values is interleaved on the device
// =================================================================================================
// The tick sequence of consecutive launches is contiguous and a member's whole state is in memory between them, so the
// split changes no result.  launch(P, io) enqueues one launch of io.n_steps steps.
template <class T, class Launch>
static int pop_run(soccer_handle* h, const T* q, int32_t n_steps, Launch launch) {
    for (int32_t t0 = 0; t0 < n_steps; t0 += q->launch_steps) {
        KernelParams P = h->P;
        auto io = q->io;
        io.n_steps = n_steps - t0 < q->launch_steps ? n_steps - t0 : q->launch_steps;
        bind_tick(h, P, (uint64_t)io.n_steps);
        HIP_TRY(h, launch(P, io));
    }
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

// what *_update of a population checks before its launch
template <class T>
static int pop_update_check(soccer_handle* h, T* q, const char* what, const uint16_t* obs, const int8_t* act_a, const int8_t* act_b,
                            const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs) {
    if (int rc = check(h, q, what)) return rc;
    if (int rc = transitions_check(h, what, true, obs, act_a, act_b, reward, terminated, next_obs)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return SOCCER_OK;
}

// the grid of a population's run / update launch: grid_for, under the population's own cap where it has one
// (SOCCER_POP_GRID_BLOCKS, read at creation: 1 .. the handle's grid_cap, ignored otherwise — tests: a grid-stride loop over
// members that wraps on a small population, as SOCCER_MQ_POP_WAVES does for the minimax-Q population)
static int pop_grid(const soccer_handle* h, int grid_blocks, uint64_t members) {
    const int g = grid_for(h, members);
    return grid_blocks > 0 && g > grid_blocks ? grid_blocks : g;
}

// The device keeps the values of a state side by side in a row of `row` float64 slots, [member][state][row]; the caller has
// an array [member][state][width] per part.  read / load move members first .. first + count through a host staging block.
struct PopTable { double* tab; size_t nS, row; };
enum Row0 { kRow0Zero, kRow0Keep, kRow0Copy };   // what a load does to state 0 of a part: writes 0 (Q, V), leaves what creation
                                                 // gave (the strategies), takes the caller's (a count)
template <class V>
struct RowPart { V* host; int slot, width; Row0 row0; };   // host NULL: not asked for / not given; 8-byte values of any type

// members per pass through the staging block (32 MB of interleaved rows at most, one member at least)
static size_t pop_chunk(const PopTable& t) { return std::max<size_t>(1, (size_t(32) << 20) / (t.nS * t.row * 8)); }

template <size_t N>
static int pop_rows_read(soccer_handle* h, const PopTable& t, int64_t first, int64_t count, const RowPart<void> (&parts)[N]) {
    if (std::none_of(parts, parts + N, [](const RowPart<void>& p) { return p.host != nullptr; })) return SOCCER_OK;
    const size_t per = t.nS * t.row, chunk = pop_chunk(t);
    std::vector<double> stage;
    for (size_t m0 = 0; m0 < (size_t)count; m0 += chunk) {
        const size_t m = std::min(chunk, (size_t)count - m0);
        stage.resize(m * per);
        HIP_TRY(h, hipMemcpy(stage.data(), t.tab + ((size_t)first + m0) * per, m * per * 8, hipMemcpyDeviceToHost));
        for (size_t r = 0; r < m * t.nS; ++r)
            for (const RowPart<void>& p : parts)
                if (p.host)
                    std::memcpy((char*)p.host + (m0 * t.nS + r) * (size_t)p.width * 8, stage.data() + r * t.row + p.slot, (size_t)p.width * 8);
    }
    return SOCCER_OK;
}

// What is not given stays: unless the parts overwrite every slot of every row, a chunk is read before it is written.
template <size_t N>
static int pop_rows_load(soccer_handle* h, const PopTable& t, int64_t first, int64_t count, const RowPart<const void> (&parts)[N]) {
    size_t given = 0, written = 0;
    for (const RowPart<const void>& p : parts)
        if (p.host) { given += 1; written += p.row0 != kRow0Keep ? (size_t)p.width : 0; }
    if (!given) return SOCCER_OK;
    const size_t per = t.nS * t.row, chunk = pop_chunk(t);
    std::vector<double> stage;
    for (size_t m0 = 0; m0 < (size_t)count; m0 += chunk) {
        const size_t m = std::min(chunk, (size_t)count - m0);
        double* const dev = t.tab + ((size_t)first + m0) * per;
        stage.resize(m * per);
        if (written != t.row) HIP_TRY(h, hipMemcpy(stage.data(), dev, m * per * 8, hipMemcpyDeviceToHost));
        for (size_t r = 0; r < m * t.nS; ++r) {
            const bool row0 = r % t.nS == 0;
            for (const RowPart<const void>& p : parts) {
                if (!p.host || (row0 && p.row0 == kRow0Keep)) continue;
                double* const to = stage.data() + r * t.row + p.slot;
                if (row0 && p.row0 == kRow0Zero) std::memset(to, 0, (size_t)p.width * 8);
                else std::memcpy(to, (const char*)p.host + (m0 * t.nS + r) * (size_t)p.width * 8, (size_t)p.width * 8);
            }
        }
        HIP_TRY(h, hipMemcpy(dev, stage.data(), m * per * 8, hipMemcpyHostToDevice));
    }
    return SOCCER_OK;
}

// ---- populations of independent Q-learners: soccer_q_population_* ---------------------------------
static_assert(kPopGreedy == SOCCER_QL_GREEDY && kPopUniform == SOCCER_QL_UNIFORM, "the kernels' names of the modes");

// what soccer_q_population_create_league adds to a creation: the league's player, its K policies and their weights (HOST)
struct PopLeagueSpec {
    int32_t player, K;
    const double* policies;             // [K][nS][5]
    const double* weights;              // [K]
};

// both creations; `what` names the entry point in the messages, lg == nullptr: no league
static int pop_create(soccer_handle* h, const soccer_q_population_config* cfg, const PopLeagueSpec* lg, const char* what,
                      soccer_q_population** out) {
    if (int rc = create_check(h, cfg, out, what)) return rc;
    const size_t n = (size_t)h->cfg.n_lanes;
    std::vector<double> par[4];         // alpha, decay, explor, discount_factor
    if (int rc = pop_params(h, cfg, n, par)) return rc;
    if (!ql_kind(cfg->act_a) || !ql_kind(cfg->act_b))
        return fail(h, SOCCER_E_INVALID, "act_a / act_b must be SOCCER_QL_GREEDY, SOCCER_QL_UNIFORM or SOCCER_QL_FIXED");
    const int nS = h->rules.nS;
    // the league player is SOCCER_QL_FIXED with a NULL policy: its rows come from the league
    const bool league_a = lg && lg->player == 0, league_b = lg && lg->player == 1;
    if (lg) {
        if (!league_a && !league_b) return fail(h, SOCCER_E_INVALID, "%s: league_player must be 0 (player A) or 1 (player B)", what);
        if ((league_a ? cfg->act_a : cfg->act_b) != SOCCER_QL_FIXED || (league_a ? cfg->policy_a : cfg->policy_b) != nullptr)
            return fail(h, SOCCER_E_INVALID, "%s: the league player must be SOCCER_QL_FIXED with a NULL policy (act_%c / policy_%c)", what,
                        league_a ? 'a' : 'b', league_a ? 'a' : 'b');
        if (lg->K < 1 || lg->K > SOCCER_LEAGUE_MAX_POLICIES)
            return fail(h, SOCCER_E_INVALID, "%s: n_policies must be in 1 .. %d, not %d", what, SOCCER_LEAGUE_MAX_POLICIES, (int)lg->K);
        if (!lg->policies || !lg->weights) return fail(h, SOCCER_E_INVALID, "%s: policies / weights is NULL", what);
    }
    if (!league_a && (cfg->act_a == SOCCER_QL_FIXED) != (cfg->policy_a != nullptr)) return fail(h, SOCCER_E_INVALID, "policy_a goes with act_a == SOCCER_QL_FIXED, and only with it");
    if (!league_b && (cfg->act_b == SOCCER_QL_FIXED) != (cfg->policy_b != nullptr)) return fail(h, SOCCER_E_INVALID, "policy_b goes with act_b == SOCCER_QL_FIXED, and only with it");
    std::vector<uint16_t> fixed[2];
    if (cfg->policy_a) if (int rc = thresholds(h, "policy_a", cfg->policy_a, nS, fixed[0])) return rc;
    if (cfg->policy_b) if (int rc = thresholds(h, "policy_b", cfg->policy_b, nS, fixed[1])) return rc;
    std::vector<uint16_t> league_thr;   // [K][nS][4]
    std::vector<uint64_t> league_T;     // [K - 1]
    if (lg) {
        const int bad = league_check_weights(lg->weights, lg->K);
        if (bad >= 0 && bad < lg->K) return fail(h, SOCCER_E_INVALID, "weights[%d] is negative or not a finite number", bad);
        if (bad == lg->K) return fail(h, SOCCER_E_INVALID, "weights does not sum to 1");
        league_thr.reserve((size_t)lg->K * (size_t)nS * 4);
        char name[48];
        for (int k = 0; k < lg->K; ++k) {
            std::snprintf(name, sizeof name, "policies[%d]", k);
            if (int rc = thresholds(h, name, lg->policies + (size_t)k * (size_t)nS * 5, nS, league_thr)) return rc;
        }
        league_T.assign((size_t)std::max(lg->K - 1, 1), 0);        // (K == 1: one unread entry, so that no pointer is NULL)
        league_thresholds(lg->weights, lg->K, league_T.data());
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, with_shape(h, [&](auto slip, auto lds) {
        return lg ? raise_lds_limit(h, pop_league_run_kernel<slip, lds>) : raise_lds_limit(h, pop_run_kernel<slip, lds>);
    }));
    std::unique_ptr<soccer_q_population> owner(new soccer_q_population(h));
    soccer_q_population* q = owner.get();
    q->grid_blocks = (int)env_in("SOCCER_POP_GRID_BLOCKS", 1, h->grid_cap, 0);
    PopIO& io = q->io;
    double* dpar[4] = {nullptr, nullptr, nullptr, nullptr};
    uint16_t* dmix[2] = {nullptr, nullptr};
    int rc = q->bufs.alloc(h, n * (size_t)nS * 10, &io.Q);     // (a failure frees what was taken: `owner` goes, the handle is as it was)
    for (int k = 0; k < 4; ++k) if (!rc) rc = q->bufs.alloc(h, n, &dpar[k]);
    for (int p = 0; p < 2; ++p) if (!rc && !fixed[p].empty()) rc = q->bufs.alloc(h, (size_t)nS * 4, &dmix[p]);
    if (!rc) rc = q->bufs.alloc(h, 1, &io.steps);
    uint16_t* dthr = nullptr; uint64_t* dT = nullptr; int32_t* dpick = nullptr;
    if (lg) {
        if (!rc) rc = q->bufs.alloc(h, league_thr.size(), &dthr);
        if (!rc) rc = q->bufs.alloc(h, league_T.size(), &dT);
        if (!rc) rc = q->bufs.alloc(h, n, &dpick);
    }
    if (rc) return rc;
    io.alpha = dpar[0]; io.decay = dpar[1]; io.explor = dpar[2]; io.gamma = dpar[3];
    io.mix[0] = dmix[0]; io.mix[1] = dmix[1];
    io.misuse = h->d_misuse;
    io.nS = nS; io.n_steps = 0;
    io.mode[0] = cfg->act_a; io.mode[1] = cfg->act_b;
    for (int k = 0; k < 4; ++k) HIP_TRY(h, hipMemcpyAsync(dpar[k], par[k].data(), n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    for (int p = 0; p < 2; ++p)
        if (dmix[p]) HIP_TRY(h, hipMemcpyAsync(dmix[p], fixed[p].data(), fixed[p].size() * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
    if (lg) {
        q->league = PopLeagueIO{dthr, dT, dpick, lg->K, lg->player};
        HIP_TRY(h, hipMemcpyAsync(dthr, league_thr.data(), league_thr.size() * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(dT, league_T.data(), league_T.size() * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemsetAsync(dpick, 0xff, n * sizeof(int32_t), h->stream));         // every pick -1
    }
    hipLaunchKernelGGL(pop_init_kernel, dim3(grid_for(h, (uint64_t)n * (uint64_t)nS * 10)), dim3(kBlock), 0, h->stream, io, (unsigned long long)n, cfg->q_init);
    return created(owner, out);
}

extern "C" int soccer_q_population_create(soccer_handle* h, const soccer_q_population_config* cfg, soccer_q_population** out) {
    return pop_create(h, cfg, nullptr, "soccer_q_population_create", out);
}

extern "C" int soccer_q_population_create_league(soccer_handle* h, const soccer_q_population_config* cfg, int32_t league_player,
                                                 int32_t n_policies, const double* policies, const double* weights,
                                                 soccer_q_population** out) {
    const PopLeagueSpec lg{league_player, n_policies, policies, weights};
    return pop_create(h, cfg, &lg, "soccer_q_population_create_league", out);
}

static int pop_league_check(soccer_handle* h, soccer_q_population* q, const char* what, int64_t first, int64_t count) {
    if (int rc = check(h, q, what)) return rc;
    if (q->league.K == 0) return fail(h, SOCCER_E_INVALID, "%s: this population has no league (soccer_q_population_create_league)", what);
    return range_check(h, q, what, first, count);
}

extern "C" int soccer_q_population_league_read(soccer_handle* h, soccer_q_population* q, int64_t first, int64_t count, int32_t* pick) {
    if (int rc = pop_league_check(h, q, "soccer_q_population_league_read", first, count)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (pick && count) HIP_TRY(h, hipMemcpyAsync(pick, q->league.pick + first, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SOCCER_OK;
}

extern "C" int soccer_q_population_league_load(soccer_handle* h, soccer_q_population* q, int64_t first, int64_t count, const int32_t* pick) {
    if (int rc = pop_league_check(h, q, "soccer_q_population_league_load", first, count)) return rc;
    if (!pick && count) return fail(h, SOCCER_E_INVALID, "soccer_q_population_league_load: pick is NULL");
    // everything is checked before anything is written: the kernel uses a pick as an index
    for (int64_t i = 0; i < count; ++i)
        if (pick[i] < -1 || pick[i] >= q->league.K)
            return fail(h, SOCCER_E_INVALID, "soccer_q_population_league_load: pick[%lld] = %d is outside -1 .. %d", (long long)i, (int)pick[i],
                        (int)q->league.K - 1);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (count) HIP_TRY(h, hipMemcpy(q->league.pick + first, pick, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice));
    return SOCCER_OK;
}

extern "C" int soccer_q_population_destroy(soccer_handle* h, soccer_q_population* q) { return destroy(h, q, "soccer_q_population_destroy"); }

extern "C" int soccer_q_population_run(soccer_handle* h, soccer_q_population* q, int32_t n_steps) {
    if (int rc = run_check(h, q, n_steps, "soccer_q_population_run")) return rc;
    // (a league's kick-off draws take the blocks of counter 2^62 + tick: below 2^62 a tick's own blocks are never met)
    if (q->league.K != 0 && (h->tick >= (1ull << 62) || (uint64_t)n_steps > (1ull << 62) - h->tick))
        return fail(h, SOCCER_E_INVALID, "soccer_q_population_run: a league population's run may not cross tick 2^62");
    return pop_run(h, q, n_steps, [&](const KernelParams& P, const PopIO& io) {
        return with_shape(h, [&](auto slip, auto lds) {
            const dim3 grid(pop_grid(h, q->grid_blocks, P.n));
            if (q->league.K != 0) hipLaunchKernelGGL((pop_league_run_kernel<slip, lds>), grid, dim3(kBlock), h->smem_bytes, h->stream, P, io, q->league);
            else hipLaunchKernelGGL((pop_run_kernel<slip, lds>), grid, dim3(kBlock), h->smem_bytes, h->stream, P, io);
            return hipSuccess;
        });
    });
}

extern "C" int soccer_q_population_update(soccer_handle* h, soccer_q_population* q, const uint16_t* obs, const int8_t* act_a,
                                          const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs) {
    if (int rc = pop_update_check(h, q, "soccer_q_population_update", obs, act_a, act_b, reward, terminated, next_obs)) return rc;
    hipLaunchKernelGGL(pop_update_kernel, dim3(pop_grid(h, q->grid_blocks, (uint64_t)q->n)), dim3(kBlock), 0, h->stream, q->io, (long long)q->n,
                       obs, act_a, act_b, reward, terminated, next_obs);
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

extern "C" int soccer_q_population_read(soccer_handle* h, soccer_q_population* q, int64_t first, int64_t count, double* Q_a, double* Q_b,
                                        double* alpha, uint64_t* steps) {
    if (int rc = check(h, q, "soccer_q_population_read")) return rc;
    if (int rc = range_check(h, q, "soccer_q_population_read", first, count)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const PopIO& io = q->io;
    if (alpha && count) HIP_TRY(h, hipMemcpyAsync(alpha, io.alpha + first, (size_t)count * 8, hipMemcpyDeviceToHost, h->stream));
    if (steps) HIP_TRY(h, hipMemcpyAsync(steps, io.steps, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const RowPart<void> parts[2] = {{Q_a, 0, 5, kRow0Zero}, {Q_b, 5, 5, kRow0Zero}};
    return pop_rows_read(h, PopTable{io.Q, (size_t)io.nS, 10}, first, count, parts);
}

extern "C" int soccer_q_population_load(soccer_handle* h, soccer_q_population* q, int64_t first, int64_t count, const double* Q_a,
                                        const double* Q_b, const double* alpha, const uint64_t* steps) {
    if (int rc = check(h, q, "soccer_q_population_load")) return rc;
    if (int rc = range_check(h, q, "soccer_q_population_load", first, count)) return rc;
    const PopIO& io = q->io;
    const size_t nS = (size_t)io.nS;
    // everything is checked before anything is written
    if (Q_a && count) if (int rc = bounds_check(h, "soccer_q_population_load", "Q_a", Q_a, (size_t)count, nS, 5)) return rc;
    if (Q_b && count) if (int rc = bounds_check(h, "soccer_q_population_load", "Q_b", Q_b, (size_t)count, nS, 5)) return rc;
    if (alpha) if (int rc = unit_check(h, "soccer_q_population_load", "alpha", alpha, (size_t)count)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const RowPart<const void> parts[2] = {{Q_a, 0, 5, kRow0Zero}, {Q_b, 5, 5, kRow0Zero}};   // (one alone: the other player's rows stay)
    if (int rc = pop_rows_load(h, PopTable{io.Q, nS, 10}, first, count, parts)) return rc;
    if (alpha && count) HIP_TRY(h, hipMemcpy(io.alpha + first, alpha, (size_t)count * 8, hipMemcpyHostToDevice));
    if (steps) HIP_TRY(h, hipMemcpy(io.steps, steps, 8, hipMemcpyHostToDevice));
    return SOCCER_OK;
}

// ---- populations of policy hill-climbers: soccer_wolf_population_* --------------------------------
static_assert(kPhcLearn == SOCCER_PHC_LEARN && kPhcUniform == SOCCER_PHC_UNIFORM && kPhcFixed == SOCCER_PHC_FIXED, "the kernels' names of the modes");

static void launch_adopt(soccer_handle* h, double* dst, int dst_slot, const double* src, size_t src_member, size_t src_row, size_t first,
                         size_t count, int nS) {
    if (count)
        hipLaunchKernelGGL(phc_pop_adopt_kernel, dim3(grid_for(h, (uint64_t)count * (uint64_t)nS)), dim3(kBlock), 0, h->stream, dst, dst_slot, src,
                           (unsigned long long)src_member, (unsigned long long)src_row, (unsigned long long)first, (unsigned long long)count,
                           (int32_t)nS);
}

extern "C" int soccer_wolf_population_create(soccer_handle* h, const soccer_wolf_population_config* cfg, soccer_wolf_population** out) {
    if (int rc = create_check(h, cfg, out, "soccer_wolf_population_create")) return rc;
    const size_t n = (size_t)h->cfg.n_lanes;
    std::vector<double> par[7];         // alpha, decay, explor, discount_factor, delta_win, delta_lose, delta_decay
    if (int rc = pop_params(h, cfg, n, par)) return rc;
    if (int rc = pop_param(h, "delta_win", "[0, 1]", cfg->delta_win_per_member, cfg->delta_win, n, in_unit, par[4])) return rc;
    if (int rc = pop_param(h, "delta_lose", "[0, 1]", cfg->delta_lose_per_member, cfg->delta_lose, n, in_unit, par[5])) return rc;
    if (int rc = pop_param(h, "delta_decay", "(0, 1]", cfg->delta_decay_per_member, cfg->delta_decay, n, in_factor, par[6])) return rc;
    if (!phc_kind(cfg->act_a) || !phc_kind(cfg->act_b))
        return fail(h, SOCCER_E_INVALID, "act_a / act_b must be SOCCER_PHC_LEARN, SOCCER_PHC_UNIFORM or SOCCER_PHC_FIXED");
    const int nS = h->rules.nS;
    const int32_t kinds[2] = {cfg->act_a, cfg->act_b};
    const double* shared[2] = {cfg->policy_a, cfg->policy_b};
    const double* each[2] = {cfg->policy_a_per_member, cfg->policy_b_per_member};
    static const char* const names[2][2] = {{"policy_a", "policy_a_per_member"}, {"policy_b", "policy_b_per_member"}};
    for (int p = 0; p < 2; ++p) {
        if ((kinds[p] == SOCCER_PHC_FIXED) != ((shared[p] != nullptr) != (each[p] != nullptr)) || (shared[p] && each[p]))
            return fail(h, SOCCER_E_INVALID, "exactly one of %s and %s goes with act_%c == SOCCER_PHC_FIXED, and neither with another mode",
                        names[p][0], names[p][1], p ? 'b' : 'a');
        // (row 0 included, as a fixed policy's thresholds check it; a shared policy is member 0 of one)
        if (shared[p]) if (int rc = rows_check(h, "soccer_wolf_population_create", names[p][0], shared[p], 1, nS, 0)) return rc;
        if (each[p]) if (int rc = rows_check(h, "soccer_wolf_population_create", names[p][1], each[p], n, nS, 0)) return rc;
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, with_shape(h, [&](auto slip, auto lds) { return raise_lds_limit(h, phc_pop_run_kernel<slip, lds>); }));
    std::unique_ptr<soccer_wolf_population> owner(new soccer_wolf_population(h));
    soccer_wolf_population* q = owner.get();
    q->grid_blocks = (int)env_in("SOCCER_POP_GRID_BLOCKS", 1, h->grid_cap, 0);
    PhcPopIO& io = q->io;
    double* dpar[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t per = (size_t)nS * kPhcRow, chunk = std::min(pop_chunk(PopTable{nullptr, (size_t)nS, kPhcRow}), n);
    OwnedBufs stage_bufs{"the fixed policies of a population"};          // creation's staging block: freed when this call returns
    double* stage = nullptr;
    int rc = q->bufs.alloc(h, n * per, &io.tab);               // (a failure frees what was taken: `owner` goes, the handle is as it was)
    for (int k = 0; k < 7; ++k) if (!rc) rc = q->bufs.alloc(h, n, &dpar[k]);
    if (!rc) rc = q->bufs.alloc(h, n, &io.dscale);
    if (!rc) rc = q->bufs.alloc(h, 1, &io.steps);
    if (!rc && (shared[0] || shared[1] || each[0] || each[1])) rc = stage_bufs.alloc(h, chunk * (size_t)nS * 5, &stage);
    if (rc) return rc;
    io.alpha = dpar[0]; io.decay = dpar[1]; io.explor = dpar[2]; io.gamma = dpar[3];
    io.delta_win = dpar[4]; io.delta_lose = dpar[5]; io.delta_decay = dpar[6];
    io.misuse = h->d_misuse;
    io.nS = nS; io.n_steps = 0;
    io.mode[0] = cfg->act_a; io.mode[1] = cfg->act_b;
    for (int k = 0; k < 7; ++k) HIP_TRY(h, hipMemcpyAsync(dpar[k], par[k].data(), n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(phc_pop_init_kernel, dim3(grid_for(h, (uint64_t)n * (uint64_t)per)), dim3(kBlock), 0, h->stream, io, (unsigned long long)n, cfg->q_init);
    for (int p = 0; p < 2; ++p) {
        const int slot = kPhcPi + p * kPhcPlayer;
        if (shared[p]) {
            HIP_TRY(h, hipMemcpyAsync(stage, shared[p], (size_t)nS * 40, hipMemcpyHostToDevice, h->stream));
            launch_adopt(h, io.tab, slot, stage, 0, 5, 0, n, nS);
            HIP_TRY(h, hipStreamSynchronize(h->stream));        // the staging block is used again
        }
        if (each[p])
            for (size_t m0 = 0; m0 < n; m0 += chunk) {
                const size_t m = std::min(chunk, n - m0);
                HIP_TRY(h, hipMemcpyAsync(stage, each[p] + m0 * (size_t)nS * 5, m * (size_t)nS * 40, hipMemcpyHostToDevice, h->stream));
                launch_adopt(h, io.tab, slot, stage, (size_t)nS * 5, 5, m0, m, nS);
                HIP_TRY(h, hipStreamSynchronize(h->stream));
            }
    }
    return created(owner, out);
}

extern "C" int soccer_wolf_population_destroy(soccer_handle* h, soccer_wolf_population* q) {
    return destroy(h, q, "soccer_wolf_population_destroy");
}

extern "C" int soccer_wolf_population_run(soccer_handle* h, soccer_wolf_population* q, int32_t n_steps) {
    if (int rc = run_check(h, q, n_steps, "soccer_wolf_population_run")) return rc;
    return pop_run(h, q, n_steps, [&](const KernelParams& P, const PhcPopIO& io) {
        return with_shape(h, [&](auto slip, auto lds) {
            hipLaunchKernelGGL((phc_pop_run_kernel<slip, lds>), dim3(pop_grid(h, q->grid_blocks, P.n)), dim3(kBlock), h->smem_bytes, h->stream, P, io);
            return hipSuccess;
        });
    });
}

extern "C" int soccer_wolf_population_update(soccer_handle* h, soccer_wolf_population* q, const uint16_t* obs, const int8_t* act_a,
                                             const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs) {
    if (int rc = pop_update_check(h, q, "soccer_wolf_population_update", obs, act_a, act_b, reward, terminated, next_obs)) return rc;
    hipLaunchKernelGGL(phc_pop_update_kernel, dim3(pop_grid(h, q->grid_blocks, (uint64_t)q->n)), dim3(kBlock), 0, h->stream, q->io, (long long)q->n,
                       obs, act_a, act_b, reward, terminated, next_obs);
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

extern "C" int soccer_wolf_population_read(soccer_handle* h, soccer_wolf_population* q, int64_t first, int64_t count,
                                           const soccer_wolf_population_state* out) {
    if (int rc = check(h, q, "soccer_wolf_population_read")) return rc;
    if (int rc = range_check(h, q, "soccer_wolf_population_read", first, count)) return rc;
    if (!out) return fail(h, SOCCER_E_INVALID, "soccer_wolf_population_read: out is NULL");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const PhcPopIO& io = q->io;
    if (out->alpha && count) HIP_TRY(h, hipMemcpyAsync(out->alpha, io.alpha + first, (size_t)count * 8, hipMemcpyDeviceToHost, h->stream));
    if (out->dscale && count) HIP_TRY(h, hipMemcpyAsync(out->dscale, io.dscale + first, (size_t)count * 8, hipMemcpyDeviceToHost, h->stream));
    if (out->steps) HIP_TRY(h, hipMemcpyAsync(out->steps, io.steps, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const RowPart<void> parts[7] = {{out->Q_a, 0, 5, kRow0Zero}, {out->Q_b, 5, 5, kRow0Zero},
                                    {out->pi_a, kPhcPi, 5, kRow0Keep}, {out->pi_b, kPhcPi + kPhcPlayer, 5, kRow0Keep},
                                    {out->avg_a, kPhcAvg, 5, kRow0Keep}, {out->avg_b, kPhcAvg + kPhcPlayer, 5, kRow0Keep},
                                    {out->updates, kPhcUpdates, 1, kRow0Copy}};
    return pop_rows_read(h, PopTable{io.tab, (size_t)io.nS, kPhcRow}, first, count, parts);
}

extern "C" int soccer_wolf_population_load(soccer_handle* h, soccer_wolf_population* q, int64_t first, int64_t count,
                                           const soccer_wolf_population_state* in) {
    static const char* const what = "soccer_wolf_population_load";
    if (int rc = check(h, q, what)) return rc;
    if (int rc = range_check(h, q, what, first, count)) return rc;
    if (!in) return fail(h, SOCCER_E_INVALID, "soccer_wolf_population_load: in is NULL");
    const PhcPopIO& io = q->io;
    const size_t nS = (size_t)io.nS;
    // a UNIFORM player keeps its constant rows
    const bool has[2] = {io.mode[0] != kPhcUniform, io.mode[1] != kPhcUniform};
    const double* rows[6] = {in->Q_a, in->Q_b, has[0] ? in->pi_a : nullptr, has[1] ? in->pi_b : nullptr,
                             has[0] ? in->avg_a : nullptr, has[1] ? in->avg_b : nullptr};
    static const char* const names[6] = {"Q_a", "Q_b", "pi_a", "pi_b", "avg_a", "avg_b"};
    // everything is checked before anything is written
    for (int i = 0; i < 2; ++i)
        if (rows[i] && count) if (int rc = bounds_check(h, what, names[i], rows[i], (size_t)count, nS, 5)) return rc;
    for (int i = 2; i < 6; ++i)
        if (rows[i]) if (int rc = rows_check(h, what, names[i], rows[i], (size_t)count, io.nS, 1)) return rc;
    if (in->alpha) if (int rc = unit_check(h, what, "alpha", in->alpha, (size_t)count)) return rc;
    if (in->dscale) if (int rc = unit_check(h, what, "dscale", in->dscale, (size_t)count)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const RowPart<const void> parts[7] = {{rows[0], 0, 5, kRow0Zero}, {rows[1], 5, 5, kRow0Zero},
                                          {rows[2], kPhcPi, 5, kRow0Keep}, {rows[3], kPhcPi + kPhcPlayer, 5, kRow0Keep},
                                          {rows[4], kPhcAvg, 5, kRow0Keep}, {rows[5], kPhcAvg + kPhcPlayer, 5, kRow0Keep},
                                          {in->updates, kPhcUpdates, 1, kRow0Copy}};
    if (int rc = pop_rows_load(h, PopTable{io.tab, nS, kPhcRow}, first, count, parts)) return rc;
    if (in->alpha && count) HIP_TRY(h, hipMemcpy(io.alpha + first, in->alpha, (size_t)count * 8, hipMemcpyHostToDevice));
    if (in->dscale && count) HIP_TRY(h, hipMemcpy(io.dscale + first, in->dscale, (size_t)count * 8, hipMemcpyHostToDevice));
    if (in->steps) HIP_TRY(h, hipMemcpy(io.steps, in->steps, 8, hipMemcpyHostToDevice));
    return SOCCER_OK;
}

extern "C" int soccer_wolf_population_adopt(soccer_handle* h, soccer_wolf_population* dst, int32_t dst_player, soccer_wolf_population* src,
                                            int32_t src_player, int32_t which) {
    if (int rc = check(h, dst, "soccer_wolf_population_adopt (dst)")) return rc;
    if (int rc = check(h, src, "soccer_wolf_population_adopt (src)")) return rc;
    if (src == dst) return fail(h, SOCCER_E_INVALID, "soccer_wolf_population_adopt: src and dst are the same population");
    if ((dst_player != 0 && dst_player != 1) || (src_player != 0 && src_player != 1))
        return fail(h, SOCCER_E_INVALID, "soccer_wolf_population_adopt: dst_player / src_player must be 0 (player A) or 1 (player B)");
    if (which != 0 && which != 1) return fail(h, SOCCER_E_INVALID, "soccer_wolf_population_adopt: which must be 0 (pi) or 1 (avg)");
    if (dst->io.mode[dst_player] != kPhcFixed)
        return fail(h, SOCCER_E_INVALID, "soccer_wolf_population_adopt: player %c of dst is not SOCCER_PHC_FIXED", dst_player ? 'B' : 'A');
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t nS = (size_t)dst->io.nS;                   // (one handle: the same pitch, the same number of members)
    launch_adopt(h, dst->io.tab, kPhcPi + dst_player * kPhcPlayer, src->io.tab + (which ? kPhcAvg : kPhcPi) + src_player * kPhcPlayer,
                 nS * kPhcRow, kPhcRow, 0, (size_t)dst->n, (int)nS);
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

// ---- populations of minimax-Q learners: soccer_minimax_q_population_* -----------------------------
static_assert(kMqUniform == SOCCER_MQ_UNIFORM && kMqSelf == SOCCER_MQ_SELF && kMqFixed == SOCCER_MQ_FIXED, "the kernels' names of the modes");

// workgroups of one wave for `items` members (or states): never more than the population's histogram slots allow
static unsigned mqpop_grid(const soccer_minimax_q_population* q, uint64_t items) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(items, q->waves));
}

extern "C" int soccer_minimax_q_population_create(soccer_handle* h, const soccer_minimax_q_population_config* cfg,
                                                  soccer_minimax_q_population** out) {
    if (int rc = create_check(h, cfg, out, "soccer_minimax_q_population_create")) return rc;
    const size_t n = (size_t)h->cfg.n_lanes;
    std::vector<double> par[4];         // alpha, decay, explor, discount_factor
    if (int rc = pop_params(h, cfg, n, par)) return rc;
    if (cfg->opponent != SOCCER_MQ_UNIFORM && cfg->opponent != SOCCER_MQ_SELF && cfg->opponent != SOCCER_MQ_FIXED)
        return fail(h, SOCCER_E_INVALID, "opponent must be SOCCER_MQ_UNIFORM, SOCCER_MQ_SELF or SOCCER_MQ_FIXED");
    const double* const shared = cfg->opponent_policy;
    const double* const each = cfg->opponent_policy_per_member;
    if ((cfg->opponent == SOCCER_MQ_FIXED) != ((shared != nullptr) != (each != nullptr)) || (shared && each))
        return fail(h, SOCCER_E_INVALID, "exactly one of opponent_policy and opponent_policy_per_member goes with opponent == SOCCER_MQ_FIXED, and neither with another mode");
    const int nS = h->rules.nS;
    // (row 0 included, as a fixed policy's thresholds check it; a shared policy is member 0 of one)
    if (shared) if (int rc = rows_check(h, "soccer_minimax_q_population_create", "opponent_policy", shared, 1, nS, 0)) return rc;
    if (each) if (int rc = rows_check(h, "soccer_minimax_q_population_create", "opponent_policy_per_member", each, n, nS, 0)) return rc;
    std::vector<uint16_t> fixed;
    const size_t fixed_members = shared ? 1 : (each ? n : 0);
    for (size_t m = 0; m < fixed_members; ++m)
        if (int rc = thresholds(h, "opponent_policy", (shared ? shared : each) + m * (size_t)nS * 5, nS, fixed)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    std::unique_ptr<soccer_minimax_q_population> owner(new soccer_minimax_q_population(h));
    soccer_minimax_q_population* q = owner.get();
    // a workgroup is one wave and owns one histogram slot: as many as the capped grids of the other kernels have waves
    // (SOCCER_MQ_POP_WAVES, tests: a wave that serves several members in turn)
    q->waves = (unsigned)std::min<uint64_t>((uint64_t)h->grid_cap * (kBlock / 64), h->hist_slots);
    q->waves = (unsigned)env_in("SOCCER_MQ_POP_WAVES", 1, (long)q->waves, (long)q->waves);
    MqPopIO& io = q->io;
    double* dpar[4] = {nullptr, nullptr, nullptr, nullptr};
    uint16_t* dmix = nullptr;
    const size_t per = (size_t)nS * kMqRow;
    int rc = q->bufs.alloc(h, n * per, &io.tab);               // (a failure frees what was taken: `owner` goes, the handle is as it was)
    for (int k = 0; k < 4; ++k) if (!rc) rc = q->bufs.alloc(h, n, &dpar[k]);
    if (!rc && !fixed.empty()) rc = q->bufs.alloc(h, fixed.size(), &dmix);
    if (!rc) rc = q->bufs.alloc(h, 1, &io.steps);
    if (rc) return rc;
    io.alpha = dpar[0]; io.decay = dpar[1]; io.explor = dpar[2]; io.gamma = dpar[3];
    io.mix_b = dmix; io.mix_member = each ? (unsigned long long)nS * 4ull : 0ull;
    io.misuse = h->d_misuse;
    io.nS = nS; io.n_steps = 0; io.opponent = cfg->opponent;
    for (int k = 0; k < 4; ++k) HIP_TRY(h, hipMemcpyAsync(dpar[k], par[k].data(), n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (dmix) HIP_TRY(h, hipMemcpyAsync(dmix, fixed.data(), fixed.size() * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(mq_pop_init_kernel, dim3(grid_for(h, (uint64_t)n * (uint64_t)per)), dim3(kBlock), 0, h->stream, io, (unsigned long long)n, cfg->q_init);
    return created(owner, out);
}

extern "C" int soccer_minimax_q_population_destroy(soccer_handle* h, soccer_minimax_q_population* q) {
    return destroy(h, q, "soccer_minimax_q_population_destroy");
}

extern "C" int soccer_minimax_q_population_run(soccer_handle* h, soccer_minimax_q_population* q, int32_t n_steps) {
    if (int rc = run_check(h, q, n_steps, "soccer_minimax_q_population_run")) return rc;
    return pop_run(h, q, n_steps, [&](const KernelParams& P, const MqPopIO& io) {          // (its kernel has no LDS shape)
        const dim3 grid(mqpop_grid(q, P.n));
        if (h->slip) hipLaunchKernelGGL(mq_pop_run_kernel<true>, grid, dim3(kMqBlock), 0, h->stream, P, io);
        else hipLaunchKernelGGL(mq_pop_run_kernel<false>, grid, dim3(kMqBlock), 0, h->stream, P, io);
        return hipSuccess;
    });
}

extern "C" int soccer_minimax_q_population_update(soccer_handle* h, soccer_minimax_q_population* q, const uint16_t* obs, const int8_t* act_a,
                                                  const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs) {
    if (int rc = pop_update_check(h, q, "soccer_minimax_q_population_update", obs, act_a, act_b, reward, terminated, next_obs)) return rc;
    hipLaunchKernelGGL(mq_pop_update_kernel, dim3(mqpop_grid(q, q->n)), dim3(kMqBlock), 0, h->stream, q->io, (long long)q->n,
                       obs, act_a, act_b, reward, terminated, next_obs);
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

extern "C" int soccer_minimax_q_population_read(soccer_handle* h, soccer_minimax_q_population* q, int64_t first, int64_t count, double* Q,
                                                double* V, double* pi_a, double* pi_b, double* alpha, uint64_t* steps) {
    if (int rc = check(h, q, "soccer_minimax_q_population_read")) return rc;
    if (int rc = range_check(h, q, "soccer_minimax_q_population_read", first, count)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const MqPopIO& io = q->io;
    if (alpha && count) HIP_TRY(h, hipMemcpyAsync(alpha, io.alpha + first, (size_t)count * 8, hipMemcpyDeviceToHost, h->stream));
    if (steps) HIP_TRY(h, hipMemcpyAsync(steps, io.steps, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const RowPart<void> parts[4] = {{Q, 0, 25, kRow0Zero}, {V, kMqV, 1, kRow0Zero}, {pi_a, kMqPiA, 5, kRow0Keep}, {pi_b, kMqPiB, 5, kRow0Keep}};
    return pop_rows_read(h, PopTable{io.tab, (size_t)io.nS, kMqRow}, first, count, parts);
}

extern "C" int soccer_minimax_q_population_load(soccer_handle* h, soccer_minimax_q_population* q, int64_t first, int64_t count, const double* Q,
                                                const double* V, const double* pi_a, const double* pi_b, const double* alpha,
                                                const uint64_t* steps) {
    static const char* const what = "soccer_minimax_q_population_load";
    if (int rc = check(h, q, what)) return rc;
    if (int rc = range_check(h, q, what, first, count)) return rc;
    const MqPopIO& io = q->io;
    const size_t nS = (size_t)io.nS;
    // everything is checked before anything is written
    if (Q && count) if (int rc = bounds_check(h, what, "Q", Q, (size_t)count, nS, 25)) return rc;
    if (V && count) if (int rc = bounds_check(h, what, "V", V, (size_t)count, nS, 1)) return rc;
    if (pi_a) if (int rc = rows_check(h, what, "pi_a", pi_a, (size_t)count, io.nS, 1)) return rc;
    if (pi_b) if (int rc = rows_check(h, what, "pi_b", pi_b, (size_t)count, io.nS, 1)) return rc;
    if (alpha) if (int rc = unit_check(h, what, "alpha", alpha, (size_t)count)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const RowPart<const void> parts[4] = {{Q, 0, 25, kRow0Zero}, {V, kMqV, 1, kRow0Zero}, {pi_a, kMqPiA, 5, kRow0Keep}, {pi_b, kMqPiB, 5, kRow0Keep}};
    if (int rc = pop_rows_load(h, PopTable{io.tab, nS, kMqRow}, first, count, parts)) return rc;
    if (alpha && count) HIP_TRY(h, hipMemcpy(io.alpha + first, alpha, (size_t)count * 8, hipMemcpyHostToDevice));
    if (steps) HIP_TRY(h, hipMemcpy(io.steps, steps, 8, hipMemcpyHostToDevice));
    if (Q && !V && !pi_a && !pi_b && count > 0 && nS > 1) {             // a table alone: V and the strategies follow it
        hipLaunchKernelGGL(mq_pop_solve_kernel, dim3(mqpop_grid(q, (uint64_t)count * (uint64_t)(nS - 1))), dim3(kMqBlock), 0, h->stream, io,
                           (unsigned long long)first, (unsigned long long)count);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return SOCCER_OK;
}

// ---- populations of opponent-modelling Q-learners: soccer_om_population_* --------------------------
// the parts of a member's rows as the caller sees them: Q_a, Q_b [nS][25], C_a, C_b [nS][5]
template <class V>
static void om_parts(V* Q_a, V* Q_b, V* C_a, V* C_b, RowPart<V> (&parts)[4]) {
    parts[0] = {Q_a, 0, 25, kRow0Zero}; parts[1] = {Q_b, kOmPlayer, 25, kRow0Zero};
    parts[2] = {C_a, kOmC, 5, kRow0Zero}; parts[3] = {C_b, kOmPlayer + kOmC, 5, kRow0Zero};
}

extern "C" int soccer_om_population_create(soccer_handle* h, const soccer_om_population_config* cfg, soccer_om_population** out) {
    if (int rc = create_check(h, cfg, out, "soccer_om_population_create")) return rc;
    const size_t n = (size_t)h->cfg.n_lanes;
    std::vector<double> par[4];         // alpha, decay, explor, discount_factor
    if (int rc = pop_params(h, cfg, n, par)) return rc;
    if (!ql_kind(cfg->act_a) || !ql_kind(cfg->act_b))
        return fail(h, SOCCER_E_INVALID, "act_a / act_b must be SOCCER_QL_GREEDY, SOCCER_QL_UNIFORM or SOCCER_QL_FIXED");
    if ((cfg->act_a == SOCCER_QL_FIXED) != (cfg->policy_a != nullptr)) return fail(h, SOCCER_E_INVALID, "policy_a goes with act_a == SOCCER_QL_FIXED, and only with it");
    if ((cfg->act_b == SOCCER_QL_FIXED) != (cfg->policy_b != nullptr)) return fail(h, SOCCER_E_INVALID, "policy_b goes with act_b == SOCCER_QL_FIXED, and only with it");
    const int nS = h->rules.nS;
    std::vector<uint16_t> fixed[2];
    if (cfg->policy_a) if (int rc = thresholds(h, "policy_a", cfg->policy_a, nS, fixed[0])) return rc;
    if (cfg->policy_b) if (int rc = thresholds(h, "policy_b", cfg->policy_b, nS, fixed[1])) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, with_shape(h, [&](auto slip, auto lds) { return raise_lds_limit(h, om_pop_run_kernel<slip, lds>); }));
    std::unique_ptr<soccer_om_population> owner(new soccer_om_population(h));
    soccer_om_population* q = owner.get();
    q->grid_blocks = (int)env_in("SOCCER_POP_GRID_BLOCKS", 1, h->grid_cap, 0);
    PopIO& io = q->io;
    double* dpar[4] = {nullptr, nullptr, nullptr, nullptr};
    uint16_t* dmix[2] = {nullptr, nullptr};
    int rc = q->bufs.alloc(h, n * (size_t)nS * kOmRow, &io.Q);  // (a failure frees what was taken: `owner` goes, the handle is as it was)
    for (int k = 0; k < 4; ++k) if (!rc) rc = q->bufs.alloc(h, n, &dpar[k]);
    for (int p = 0; p < 2; ++p) if (!rc && !fixed[p].empty()) rc = q->bufs.alloc(h, (size_t)nS * 4, &dmix[p]);
    if (!rc) rc = q->bufs.alloc(h, 1, &io.steps);
    if (rc) return rc;
    io.alpha = dpar[0]; io.decay = dpar[1]; io.explor = dpar[2]; io.gamma = dpar[3];
    io.mix[0] = dmix[0]; io.mix[1] = dmix[1];
    io.misuse = h->d_misuse;
    io.nS = nS; io.n_steps = 0;
    io.mode[0] = cfg->act_a; io.mode[1] = cfg->act_b;
    for (int k = 0; k < 4; ++k) HIP_TRY(h, hipMemcpyAsync(dpar[k], par[k].data(), n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    for (int p = 0; p < 2; ++p)
        if (dmix[p]) HIP_TRY(h, hipMemcpyAsync(dmix[p], fixed[p].data(), fixed[p].size() * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(om_pop_init_kernel, dim3(grid_for(h, (uint64_t)n * (uint64_t)nS * 2)), dim3(kBlock), 0, h->stream, io, (unsigned long long)n, cfg->q_init);
    return created(owner, out);
}

extern "C" int soccer_om_population_destroy(soccer_handle* h, soccer_om_population* q) { return destroy(h, q, "soccer_om_population_destroy"); }

extern "C" int soccer_om_population_run(soccer_handle* h, soccer_om_population* q, int32_t n_steps) {
    if (int rc = run_check(h, q, n_steps, "soccer_om_population_run")) return rc;
    return pop_run(h, q, n_steps, [&](const KernelParams& P, const PopIO& io) {
        return with_shape(h, [&](auto slip, auto lds) {
            hipLaunchKernelGGL((om_pop_run_kernel<slip, lds>), dim3(pop_grid(h, q->grid_blocks, P.n)), dim3(kBlock), h->smem_bytes, h->stream, P, io);
            return hipSuccess;
        });
    });
}

extern "C" int soccer_om_population_update(soccer_handle* h, soccer_om_population* q, const uint16_t* obs, const int8_t* act_a,
                                           const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs) {
    if (int rc = pop_update_check(h, q, "soccer_om_population_update", obs, act_a, act_b, reward, terminated, next_obs)) return rc;
    hipLaunchKernelGGL(om_pop_update_kernel, dim3(pop_grid(h, q->grid_blocks, (uint64_t)q->n)), dim3(kBlock), 0, h->stream, q->io, (long long)q->n,
                       obs, act_a, act_b, reward, terminated, next_obs);
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

extern "C" int soccer_om_population_read(soccer_handle* h, soccer_om_population* q, int64_t first, int64_t count, double* Q_a, double* Q_b,
                                         uint64_t* C_a, uint64_t* C_b, double* alpha, uint64_t* steps) {
    if (int rc = check(h, q, "soccer_om_population_read")) return rc;
    if (int rc = range_check(h, q, "soccer_om_population_read", first, count)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const PopIO& io = q->io;
    if (alpha && count) HIP_TRY(h, hipMemcpyAsync(alpha, io.alpha + first, (size_t)count * 8, hipMemcpyDeviceToHost, h->stream));
    if (steps) HIP_TRY(h, hipMemcpyAsync(steps, io.steps, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    RowPart<void> parts[4];
    om_parts<void>(Q_a, Q_b, C_a, C_b, parts);
    return pop_rows_read(h, PopTable{io.Q, (size_t)io.nS, kOmRow}, first, count, parts);
}

extern "C" int soccer_om_population_load(soccer_handle* h, soccer_om_population* q, int64_t first, int64_t count, const double* Q_a,
                                         const double* Q_b, const uint64_t* C_a, const uint64_t* C_b, const double* alpha,
                                         const uint64_t* steps) {
    static const char* const what = "soccer_om_population_load";
    if (int rc = check(h, q, what)) return rc;
    if (int rc = range_check(h, q, what, first, count)) return rc;
    const PopIO& io = q->io;
    const size_t nS = (size_t)io.nS;
    // everything is checked before anything is written
    if (Q_a && count) if (int rc = bounds_check(h, what, "Q_a", Q_a, (size_t)count, nS, 25)) return rc;
    if (Q_b && count) if (int rc = bounds_check(h, what, "Q_b", Q_b, (size_t)count, nS, 25)) return rc;
    if (alpha) if (int rc = unit_check(h, what, "alpha", alpha, (size_t)count)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    RowPart<const void> parts[4];
    om_parts<const void>(Q_a, Q_b, C_a, C_b, parts);
    if (int rc = pop_rows_load(h, PopTable{io.Q, nS, kOmRow}, first, count, parts)) return rc;
    if (alpha && count) HIP_TRY(h, hipMemcpy(io.alpha + first, alpha, (size_t)count * 8, hipMemcpyHostToDevice));
    if (steps) HIP_TRY(h, hipMemcpy(io.steps, steps, 8, hipMemcpyHostToDevice));
    if ((Q_a || Q_b || C_a || C_b) && count > 0) {                      // V and g of the range follow what was loaded
        hipLaunchKernelGGL(om_pop_derive_kernel, dim3(grid_for(h, (uint64_t)count * (uint64_t)nS * 2)), dim3(kBlock), 0, h->stream, io,
                           (unsigned long long)first, (unsigned long long)count);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    return SOCCER_OK;
}

// ---- populations of regret matchers: soccer_regret_population_* ------------------------------------
// (the modes are the hill-climbers': kPhcLearn / kPhcUniform / kPhcFixed, asserted above)
// the parts of a member's rows as the caller sees them; has[p]: player p LEARNs, so its R and Z move
template <class V, class U>
static void rm_parts(V* Q_a, V* Q_b, V* R_a, V* R_b, V* Z_a, V* Z_b, U* updates, const bool (&has)[2], RowPart<V> (&parts)[7]) {
    parts[0] = {Q_a, 0, 5, kRow0Zero}; parts[1] = {Q_b, 5, 5, kRow0Zero};
    parts[2] = {has[0] ? R_a : nullptr, kRmR, 5, kRow0Zero}; parts[3] = {has[1] ? R_b : nullptr, kRmR + kRmPlayer, 5, kRow0Zero};
    parts[4] = {has[0] ? Z_a : nullptr, kRmZ, 5, kRow0Zero}; parts[5] = {has[1] ? Z_b : nullptr, kRmZ + kRmPlayer, 5, kRow0Zero};
    parts[6] = {updates, kRmUpdates, 1, kRow0Copy};
}

// rows 1.. of `members` tables [nS][5] of a checkpoint: every value finite, and >= 0 where `nonneg` (members 0: one table, and
// no member index in the message, as bounds_check)
static int finite_check(soccer_handle* h, const char* what, const char* name, const double* v, size_t members, size_t nS, bool nonneg) {
    for (size_t m = 0; m < std::max<size_t>(members, 1); ++m)
        for (size_t s = 1; s < nS; ++s)
            for (size_t k = 0; k < 5; ++k) {
                const double x = v[(m * nS + s) * 5 + k];
                if (std::isfinite(x) && !(nonneg && x < 0.0)) continue;
                const char* const why = nonneg ? "negative or not a finite number" : "not a finite number";
                if (!members) return fail(h, SOCCER_E_INVALID, "%s: %s[%zu][%zu] is %s", what, name, s, k, why);
                return fail(h, SOCCER_E_INVALID, "%s: %s[%zu][%zu][%zu] is %s", what, name, m, s, k, why);
            }
    return SOCCER_OK;
}

extern "C" int soccer_regret_population_create(soccer_handle* h, const soccer_regret_population_config* cfg, soccer_regret_population** out) {
    static const char* const what = "soccer_regret_population_create";
    if (int rc = create_check(h, cfg, out, what)) return rc;
    const size_t n = (size_t)h->cfg.n_lanes;
    std::vector<double> par[4];         // alpha, decay, explor, discount_factor
    if (int rc = pop_params(h, cfg, n, par)) return rc;
    if (!phc_kind(cfg->act_a) || !phc_kind(cfg->act_b))
        return fail(h, SOCCER_E_INVALID, "act_a / act_b must be SOCCER_PHC_LEARN, SOCCER_PHC_UNIFORM or SOCCER_PHC_FIXED");
    if ((cfg->plus != 0 && cfg->plus != 1) || (cfg->linear != 0 && cfg->linear != 1))
        return fail(h, SOCCER_E_INVALID, "plus / linear must be 0 or 1");
    const int nS = h->rules.nS;
    const int32_t kinds[2] = {cfg->act_a, cfg->act_b};
    const double* shared[2] = {cfg->policy_a, cfg->policy_b};
    const double* each[2] = {cfg->policy_a_per_member, cfg->policy_b_per_member};
    static const char* const names[2][2] = {{"policy_a", "policy_a_per_member"}, {"policy_b", "policy_b_per_member"}};
    for (int p = 0; p < 2; ++p) {
        if ((kinds[p] == SOCCER_PHC_FIXED) != ((shared[p] != nullptr) != (each[p] != nullptr)) || (shared[p] && each[p]))
            return fail(h, SOCCER_E_INVALID, "exactly one of %s and %s goes with act_%c == SOCCER_PHC_FIXED, and neither with another mode",
                        names[p][0], names[p][1], p ? 'b' : 'a');
        // (row 0 included, as a fixed policy's thresholds check it; a shared policy is member 0 of one)
        if (shared[p]) if (int rc = rows_check(h, what, names[p][0], shared[p], 1, nS, 0)) return rc;
        if (each[p]) if (int rc = rows_check(h, what, names[p][1], each[p], n, nS, 0)) return rc;
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, with_shape(h, [&](auto slip, auto lds) { return raise_lds_limit(h, rm_pop_run_kernel<slip, lds>); }));
    std::unique_ptr<soccer_regret_population> owner(new soccer_regret_population(h));
    soccer_regret_population* q = owner.get();
    q->grid_blocks = (int)env_in("SOCCER_POP_GRID_BLOCKS", 1, h->grid_cap, 0);
    RmPopIO& io = q->io;
    double* dpar[4] = {nullptr, nullptr, nullptr, nullptr};
    double* dfixed[2] = {nullptr, nullptr};
    const size_t per = (size_t)nS * kPhcRow, rows = (size_t)nS * 5;
    int rc = q->bufs.alloc(h, n * per, &io.tab);               // (a failure frees what was taken: `owner` goes, the handle is as it was)
    for (int k = 0; k < 4; ++k) if (!rc) rc = q->bufs.alloc(h, n, &dpar[k]);
    for (int p = 0; p < 2; ++p)
        if (!rc && kinds[p] == SOCCER_PHC_FIXED) rc = q->bufs.alloc(h, (each[p] ? n : 1) * rows, &dfixed[p]);
    if (!rc) rc = q->bufs.alloc(h, 1, &io.steps);
    if (rc) return rc;
    io.alpha = dpar[0]; io.decay = dpar[1]; io.explor = dpar[2]; io.gamma = dpar[3];
    io.misuse = h->d_misuse;
    io.nS = nS; io.n_steps = 0;
    io.plus = cfg->plus; io.linear = cfg->linear;
    for (int p = 0; p < 2; ++p) {
        io.mode[p] = kinds[p];
        io.fixed[p] = dfixed[p];
        io.fixed_member[p] = each[p] ? (unsigned long long)rows : 0ull;
        if (dfixed[p])          // (created() waits: the caller's array is pageable host memory)
            HIP_TRY(h, hipMemcpyAsync(dfixed[p], each[p] ? each[p] : shared[p], (each[p] ? n : 1) * rows * 8, hipMemcpyHostToDevice, h->stream));
    }
    for (int k = 0; k < 4; ++k) HIP_TRY(h, hipMemcpyAsync(dpar[k], par[k].data(), n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(rm_pop_init_kernel, dim3(grid_for(h, (uint64_t)n * (uint64_t)per)), dim3(kBlock), 0, h->stream, io, (unsigned long long)n, cfg->q_init);
    return created(owner, out);
}

extern "C" int soccer_regret_population_destroy(soccer_handle* h, soccer_regret_population* q) {
    return destroy(h, q, "soccer_regret_population_destroy");
}

extern "C" int soccer_regret_population_run(soccer_handle* h, soccer_regret_population* q, int32_t n_steps) {
    if (int rc = run_check(h, q, n_steps, "soccer_regret_population_run")) return rc;
    return pop_run(h, q, n_steps, [&](const KernelParams& P, const RmPopIO& io) {
        return with_shape(h, [&](auto slip, auto lds) {
            hipLaunchKernelGGL((rm_pop_run_kernel<slip, lds>), dim3(pop_grid(h, q->grid_blocks, P.n)), dim3(kBlock), h->smem_bytes, h->stream, P, io);
            return hipSuccess;
        });
    });
}

extern "C" int soccer_regret_population_update(soccer_handle* h, soccer_regret_population* q, const uint16_t* obs, const int8_t* act_a,
                                               const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs) {
    if (int rc = pop_update_check(h, q, "soccer_regret_population_update", obs, act_a, act_b, reward, terminated, next_obs)) return rc;
    hipLaunchKernelGGL(rm_pop_update_kernel, dim3(pop_grid(h, q->grid_blocks, (uint64_t)q->n)), dim3(kBlock), 0, h->stream, q->io, (long long)q->n,
                       obs, act_a, act_b, reward, terminated, next_obs);
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

extern "C" int soccer_regret_population_read(soccer_handle* h, soccer_regret_population* q, int64_t first, int64_t count,
                                             const soccer_regret_population_state* out) {
    if (int rc = check(h, q, "soccer_regret_population_read")) return rc;
    if (int rc = range_check(h, q, "soccer_regret_population_read", first, count)) return rc;
    if (!out) return fail(h, SOCCER_E_INVALID, "soccer_regret_population_read: out is NULL");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const RmPopIO& io = q->io;
    if (out->alpha && count) HIP_TRY(h, hipMemcpyAsync(out->alpha, io.alpha + first, (size_t)count * 8, hipMemcpyDeviceToHost, h->stream));
    if (out->steps) HIP_TRY(h, hipMemcpyAsync(out->steps, io.steps, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const bool all[2] = {true, true};   // (R and Z of a player that does not learn are the zeros creation gave)
    RowPart<void> parts[7];
    rm_parts<void, void>(out->Q_a, out->Q_b, out->R_a, out->R_b, out->Z_a, out->Z_b, out->updates, all, parts);
    return pop_rows_read(h, PopTable{io.tab, (size_t)io.nS, kPhcRow}, first, count, parts);
}

extern "C" int soccer_regret_population_load(soccer_handle* h, soccer_regret_population* q, int64_t first, int64_t count,
                                             const soccer_regret_population_state* in) {
    static const char* const what = "soccer_regret_population_load";
    if (int rc = check(h, q, what)) return rc;
    if (int rc = range_check(h, q, what, first, count)) return rc;
    if (!in) return fail(h, SOCCER_E_INVALID, "soccer_regret_population_load: in is NULL");
    const RmPopIO& io = q->io;
    const size_t nS = (size_t)io.nS;
    const bool has[2] = {io.mode[0] == kPhcLearn, io.mode[1] == kPhcLearn};
    RowPart<const void> parts[7];
    rm_parts<const void, const void>(in->Q_a, in->Q_b, in->R_a, in->R_b, in->Z_a, in->Z_b, in->updates, has, parts);
    static const char* const names[6] = {"Q_a", "Q_b", "R_a", "R_b", "Z_a", "Z_b"};
    // everything is checked before anything is written
    for (int i = 0; i < 2; ++i)
        if (parts[i].host && count) if (int rc = bounds_check(h, what, names[i], (const double*)parts[i].host, (size_t)count, nS, 5)) return rc;
    for (int i = 2; i < 6; ++i)
        if (parts[i].host)
            if (int rc = finite_check(h, what, names[i], (const double*)parts[i].host, (size_t)count, nS, i >= 4 || io.plus != 0)) return rc;
    if (in->alpha) if (int rc = unit_check(h, what, "alpha", in->alpha, (size_t)count)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (int rc = pop_rows_load(h, PopTable{io.tab, nS, kPhcRow}, first, count, parts)) return rc;
    if (in->alpha && count) HIP_TRY(h, hipMemcpy(io.alpha + first, in->alpha, (size_t)count * 8, hipMemcpyHostToDevice));
    if (in->steps) HIP_TRY(h, hipMemcpy(io.steps, in->steps, 8, hipMemcpyHostToDevice));
    return SOCCER_OK;
}

// =================================================================================================
// the regret matchers of one table: soccer_regret_learner_* (a single learner on the skeleton above, as soccer_wolf_phc is; it
// stands here, after the population, because it checks a checkpoint's regrets and policy sums with the population's finite_check)
// =================================================================================================
extern "C" int soccer_regret_learner_create(soccer_handle* h, const soccer_regret_learner_config* cfg, soccer_regret_learner** out) {
    static const char* const what = "soccer_regret_learner_create";
    if (int rc = create_check(h, cfg, out, what)) return rc;
    if (int rc = single_check(h, cfg, what)) return rc;
    if (!phc_kind(cfg->act_a) || !phc_kind(cfg->act_b))
        return fail(h, SOCCER_E_INVALID, "act_a / act_b must be SOCCER_PHC_LEARN, SOCCER_PHC_UNIFORM or SOCCER_PHC_FIXED");
    if ((cfg->plus != 0 && cfg->plus != 1) || (cfg->linear != 0 && cfg->linear != 1))
        return fail(h, SOCCER_E_INVALID, "plus / linear must be 0 or 1");
    if ((cfg->act_a == SOCCER_PHC_FIXED) != (cfg->policy_a != nullptr)) return fail(h, SOCCER_E_INVALID, "policy_a goes with act_a == SOCCER_PHC_FIXED, and only with it");
    if ((cfg->act_b == SOCCER_PHC_FIXED) != (cfg->policy_b != nullptr)) return fail(h, SOCCER_E_INVALID, "policy_b goes with act_b == SOCCER_PHC_FIXED, and only with it");
    const int nS = h->rules.nS;
    const int32_t kinds[2] = {cfg->act_a, cfg->act_b};
    const double* policy[2] = {cfg->policy_a, cfg->policy_b};
    std::vector<uint16_t> fixed[2];
    if (cfg->policy_a) if (int rc = thresholds(h, "policy_a", cfg->policy_a, nS, fixed[0])) return rc;
    if (cfg->policy_b) if (int rc = thresholds(h, "policy_b", cfg->policy_b, nS, fixed[1])) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, with_shape(h, [&](auto slip, auto lds) { return raise_lds_limit(h, rm_act_kernel<slip, lds>); }));
    std::unique_ptr<soccer_regret_learner> owner(new soccer_regret_learner(h));
    soccer_regret_learner* q = owner.get();
    RmIO& io = q->io;
    const size_t cells = (size_t)nS * 25;
    double* dfixed[2] = {nullptr, nullptr};
    int rc = SOCCER_OK;                 // (a failure frees what was taken: `owner` goes, the handle is as it was)
    for (int p = 0; p < 2; ++p) {
        if (!rc) rc = q->bufs.alloc(h, (size_t)nS * 5, &io.Q[p]);
        if (!rc) rc = q->bufs.alloc(h, (size_t)nS * 5, &io.R[p]);
        if (!rc) rc = q->bufs.alloc(h, (size_t)nS * 5, &io.Z[p]);
        if (!rc) rc = q->bufs.alloc(h, (size_t)nS, &io.Vq[p]);
        if (!rc) rc = q->bufs.alloc(h, cells, &io.sv[p]);
        if (!rc && policy[p]) rc = q->bufs.alloc(h, (size_t)nS * 5, &dfixed[p]);
    }
    if (!rc) rc = q->bufs.alloc(h, cells, &io.visits);
    if (!rc) rc = q->bufs.alloc(h, (size_t)nS, &io.updates);
    if (!rc) rc = q->bufs.alloc(h, cells, &io.cnt);
    if (!rc) rc = q->bufs.alloc(h, cells, &io.rsum);
    if (!rc && cfg->act_a != SOCCER_PHC_UNIFORM) rc = q->bufs.alloc(h, (size_t)nS * 4, &io.mix_a);
    if (!rc && cfg->act_b != SOCCER_PHC_UNIFORM) rc = q->bufs.alloc(h, (size_t)nS * 4, &io.mix_b);
    if (!rc) rc = q->bufs.alloc(h, 2, &io.alpha);
    if (!rc) rc = q->bufs.alloc(h, 1, &io.steps);
    if (rc) return rc;
    io.misuse = h->d_misuse;
    io.gamma = cfg->discount_factor; io.decay = cfg->decay; io.explor = cfg->explor;
    io.nS = nS;
    io.plus = cfg->plus; io.linear = cfg->linear;
    for (int p = 0; p < 2; ++p) { io.learn[p] = kinds[p] == SOCCER_PHC_LEARN ? 1 : 0; io.fixed[p] = dfixed[p]; }
    hipLaunchKernelGGL(rm_init_kernel, dim3((unsigned)((cells + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, io, cfg->q_init, cfg->alpha);
    for (int p = 0; p < 2; ++p) {
        if (!policy[p]) continue;
        HIP_TRY(h, hipMemcpyAsync(p ? io.mix_b : io.mix_a, fixed[p].data(), fixed[p].size() * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(dfixed[p], policy[p], (size_t)nS * 40, hipMemcpyHostToDevice, h->stream));
    }
    hipLaunchKernelGGL(rm_update_kernel<1>, dim3(q_update_grid(nS)), dim3(kLearnerBlock), 0, h->stream, io, 0);
    return created(owner, out);
}

extern "C" int soccer_regret_learner_destroy(soccer_handle* h, soccer_regret_learner* q) { return destroy(h, q, "soccer_regret_learner_destroy"); }

extern "C" int soccer_regret_learner_run(soccer_handle* h, soccer_regret_learner* q, int32_t n_steps) {
    return learner_run(h, q, n_steps, "soccer_regret_learner_run");
}

extern "C" int soccer_regret_learner_update(soccer_handle* h, soccer_regret_learner* q, int64_t n, const uint16_t* obs, const int8_t* act_a,
                                            const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs) {
    if (int rc = learner_update_check(h, q, "soccer_regret_learner_update", n, obs, act_a, act_b, reward, terminated, next_obs)) return rc;
    if (n > 0)
        hipLaunchKernelGGL(rm_reduce_kernel, dim3(grid_for(h, (uint64_t)n)), dim3(kBlock), 0, h->stream, q->io, (long long)n,
                           obs, act_a, act_b, reward, terminated, next_obs);
    launch_update(q);
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

extern "C" int soccer_regret_learner_read(soccer_handle* h, soccer_regret_learner* q, const soccer_regret_learner_state* out) {
    if (int rc = check(h, q, "soccer_regret_learner_read")) return rc;
    if (!out) return fail(h, SOCCER_E_INVALID, "soccer_regret_learner_read: out is NULL");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const RmIO& io = q->io;
    const size_t nS = (size_t)io.nS;
    double* const rows[6] = {out->Q_a, out->Q_b, out->R_a, out->R_b, out->Z_a, out->Z_b};
    const double* const from[6] = {io.Q[0], io.Q[1], io.R[0], io.R[1], io.Z[0], io.Z[1]};
    for (int i = 0; i < 6; ++i)
        if (rows[i]) HIP_TRY(h, hipMemcpyAsync(rows[i], from[i], nS * 40, hipMemcpyDeviceToHost, h->stream));
    if (out->visits) HIP_TRY(h, hipMemcpyAsync(out->visits, io.visits, nS * 200, hipMemcpyDeviceToHost, h->stream));
    if (out->updates) HIP_TRY(h, hipMemcpyAsync(out->updates, io.updates, nS * 8, hipMemcpyDeviceToHost, h->stream));
    if (out->alpha) HIP_TRY(h, hipMemcpyAsync(out->alpha, io.alpha + q->slot, 8, hipMemcpyDeviceToHost, h->stream));
    if (out->steps) HIP_TRY(h, hipMemcpyAsync(out->steps, io.steps, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SOCCER_OK;
}

extern "C" int soccer_regret_learner_load(soccer_handle* h, soccer_regret_learner* q, const soccer_regret_learner_state* in) {
    static const char* const what = "soccer_regret_learner_load";
    if (int rc = check(h, q, what)) return rc;
    if (!in || !in->Q_a || !in->Q_b) return fail(h, SOCCER_E_INVALID, "soccer_regret_learner_load: in / Q_a / Q_b is NULL");
    const RmIO& io = q->io;
    const size_t nS = (size_t)io.nS;
    // R and Z of a player that does not LEARN stay the zeros creation gave them
    const double* const rows[6] = {in->Q_a, in->Q_b, io.learn[0] ? in->R_a : nullptr, io.learn[1] ? in->R_b : nullptr,
                                   io.learn[0] ? in->Z_a : nullptr, io.learn[1] ? in->Z_b : nullptr};
    double* const to[6] = {io.Q[0], io.Q[1], io.R[0], io.R[1], io.Z[0], io.Z[1]};
    static const char* const names[6] = {"Q_a", "Q_b", "R_a", "R_b", "Z_a", "Z_b"};
    // everything is checked before anything is written
    for (int i = 0; i < 2; ++i)
        if (int rc = bounds_check(h, what, names[i], rows[i], 0, nS, 5)) return rc;
    for (int i = 2; i < 6; ++i)
        if (rows[i]) if (int rc = finite_check(h, what, names[i], rows[i], 0, nS, i >= 4 || io.plus != 0)) return rc;
    if (in->alpha) if (int rc = unit_check(h, what, "alpha", in->alpha, 1)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    for (int i = 0; i < 6; ++i) {
        if (!rows[i]) continue;
        HIP_TRY(h, hipMemsetAsync(to[i], 0, 40, h->stream));                      // row 0 is taken as zeros
        HIP_TRY(h, hipMemcpyAsync(to[i] + 5, rows[i] + 5, (nS - 1) * 40, hipMemcpyHostToDevice, h->stream));
    }
    if (in->visits) HIP_TRY(h, hipMemcpyAsync(io.visits, in->visits, nS * 200, hipMemcpyHostToDevice, h->stream));
    else HIP_TRY(h, hipMemsetAsync(io.visits, 0, nS * 200, h->stream));
    if (in->updates) HIP_TRY(h, hipMemcpyAsync(io.updates, in->updates, nS * 8, hipMemcpyHostToDevice, h->stream));
    else HIP_TRY(h, hipMemsetAsync(io.updates, 0, nS * 8, h->stream));
    if (in->alpha) HIP_TRY(h, hipMemcpyAsync(io.alpha + q->slot, in->alpha, 8, hipMemcpyHostToDevice, h->stream));
    if (in->steps) HIP_TRY(h, hipMemcpyAsync(io.steps, in->steps, 8, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(rm_update_kernel<1>, dim3(q_update_grid(io.nS)), dim3(kLearnerBlock), 0, h->stream, io, q->slot);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // the caller's arrays are pageable host memory
    return SOCCER_OK;
}
