// soccer_learners.hip — the minimax-Q learner: soccer_minimax_q_*, the independent Q-learners: soccer_q_learner_*, the
// policy hill-climbers: soccer_wolf_phc_*, the populations of one-actor Q-learners: soccer_q_population_*, the populations of
// one-actor policy hill-climbers: soccer_wolf_population_*, and the populations of one-actor minimax-Q learners:
// soccer_minimax_q_population_* (see soccer_handle.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "soccer_handle.hpp"
#include "soccer_learner_kernels.hpp"

// A learner: its device memory (one owner, like every other block of the library) and the argument block of its kernels.
// The handle lists the live ones and frees what is left when it goes.
struct soccer_minimax_q {
    soccer_handle* h = nullptr;
    LearnerIO io{};
    OwnedBufs bufs{"the minimax-Q learner"};
    int slot = 0;                       // alpha slot the NEXT update reads
};

static bool owns(const soccer_handle* h, const soccer_minimax_q* q) {
    return q && std::find(h->learners.begin(), h->learners.end(), q) != h->learners.end();
}

// The independent Q-learners of both players: the same shape.
struct soccer_q_learner {
    soccer_handle* h = nullptr;
    QLearnerIO io{};
    OwnedBufs bufs{"the Q-learner"};
    int slot = 0;                       // alpha slot the NEXT update reads
};

// The policy hill-climbers of both players: the same shape.
struct soccer_wolf_phc {
    soccer_handle* h = nullptr;
    PhcIO io{};
    OwnedBufs bufs{"the WoLF-PHC learner"};
    int slot = 0;                       // alpha / dscale slot the NEXT update reads
};

// A population of Q-learners, a member per lane: the same shape; alpha lives per member in device memory, no slots.
struct soccer_q_population {
    soccer_handle* h = nullptr;
    PopIO io{};
    OwnedBufs bufs{"the population of Q-learners"};
    unsigned long long n = 0;           // members = the handle's lanes
    int launch_steps = 4096;            // steps per pop_run_kernel launch (SOCCER_POP_LAUNCH_STEPS)
    int grid_blocks = 0;                // workgroups per run / update launch at most (SOCCER_POP_GRID_BLOCKS); 0: the handle's cap alone
    PopLeagueIO league{};               // K == 0: no league; else pop_league_run_kernel runs it
};

// A population of policy hill-climbers, a member per lane: the same shape; alpha and dscale live per member in device memory.
struct soccer_wolf_population {
    soccer_handle* h = nullptr;
    PhcPopIO io{};
    OwnedBufs bufs{"the population of WoLF-PHC learners"};
    unsigned long long n = 0;           // members = the handle's lanes
    int launch_steps = 4096;            // steps per phc_pop_run_kernel launch (SOCCER_POP_LAUNCH_STEPS)
    int grid_blocks = 0;                // workgroups per run / update launch at most (SOCCER_POP_GRID_BLOCKS); 0: the handle's cap alone
};

// A population of minimax-Q learners, a member per lane: the same shape; a member is a wave of mq_pop_run_kernel.
struct soccer_minimax_q_population {
    soccer_handle* h = nullptr;
    MqPopIO io{};
    OwnedBufs bufs{"the population of minimax-Q learners"};
    unsigned long long n = 0;           // members = the handle's lanes
    int launch_steps = 4096;            // steps per mq_pop_run_kernel launch (SOCCER_POP_LAUNCH_STEPS)
    unsigned waves = 1;                 // workgroups (of one wave) per launch at most: one episode-histogram slot each
};

void learners_release(soccer_handle* h) {
    for (soccer_minimax_q* q : h->learners) delete q;
    h->learners.clear();
    for (soccer_q_learner* q : h->q_learners) delete q;
    h->q_learners.clear();
    for (soccer_wolf_phc* q : h->phc_learners) delete q;
    h->phc_learners.clear();
    for (soccer_q_population* q : h->q_populations) delete q;
    h->q_populations.clear();
    for (soccer_wolf_population* q : h->wolf_populations) delete q;
    h->wolf_populations.clear();
    for (soccer_minimax_q_population* q : h->mq_populations) delete q;
    h->mq_populations.clear();
}

// what every entry point checks first
static int learner_check(soccer_handle* h, soccer_minimax_q* q, const char* what) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "%s during graph capture", what);
    if (!owns(h, q)) return fail(h, SOCCER_E_INVALID, "%s: not a learner of this handle", what);
    return SOCCER_OK;
}

// a fixed mixed policy's threshold rows, once: SoccerBatch.mixed_policy_thresholds
// (learner_thresholds(pi, 0.0, ...) of soccer_learner_kernels.hpp is this loop operation for operation: the populations of
// policy hill-climbers compute a FIXED player's row on the device from its pi row and get these bits — keep the two alike)
static int fixed_thresholds(soccer_handle* h, const char* name, const double* policy, int nS, std::vector<uint16_t>& rows) {
    rows.resize((size_t)nS * 4);
    for (int s = 0; s < nS; ++s) {
        const double* p = policy + (size_t)s * 5;
        double c = 0.0, sum = 0.0;
        for (int k = 0; k < 5; ++k) {
            if (!(p[k] >= 0.0)) return fail(h, SOCCER_E_INVALID, "%s[%d][%d] is negative or not a number", name, s, k);
            sum = sum + p[k];
        }
        if (!(std::fabs(sum - 1.0) <= 1e-8 + 1e-5)) return fail(h, SOCCER_E_INVALID, "%s[%d] does not sum to 1", name, s);
        for (int k = 0; k < 4; ++k) {
            c = c + p[k];
            double f = std::floor(c * 32768.0 + 1e-9);
            f = f < 0.0 ? 0.0 : (f > 32768.0 ? 32768.0 : f);
            rows[(size_t)s * 4 + k] = (uint16_t)f;
        }
    }
    return SOCCER_OK;
}

template <bool SLIP, bool LUT_LDS>
static hipError_t launch_act(soccer_handle* h, const KernelParams& P, const LearnerIO& io) {
    if (io.nS == 0)                     // soccer_minimax_q_create: the rule tables of a large pitch need more than the default LDS
        return h->smem_bytes > 48 * 1024 ? hipFuncSetAttribute(reinterpret_cast<const void*>(&learner_act_kernel<SLIP, LUT_LDS>),
                                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->smem_bytes) : hipSuccess;
    hipLaunchKernelGGL((learner_act_kernel<SLIP, LUT_LDS>), dim3(grid_for(h, P.n)), dim3(kBlock), h->smem_bytes, h->stream, P, io);
    return hipSuccess;
}

static hipError_t act(soccer_handle* h, const KernelParams& P, const LearnerIO& io) {
    return h->slip ? (h->lut_lds ? launch_act<true, true>(h, P, io) : launch_act<true, false>(h, P, io))
                   : (h->lut_lds ? launch_act<false, true>(h, P, io) : launch_act<false, false>(h, P, io));
}

static void launch_update(soccer_minimax_q* q) {
    const unsigned grid = (unsigned)((q->io.nS + kLearnerWaves - 1) / kLearnerWaves);
    hipLaunchKernelGGL(learner_update_kernel<0>, dim3(grid), dim3(kLearnerBlock), 0, q->h->stream, q->io, q->slot);
    q->slot ^= 1;
}

extern "C" int soccer_minimax_q_create(soccer_handle* h, const soccer_minimax_q_config* cfg, soccer_minimax_q** out) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_minimax_q_create during graph capture");
    if (!cfg || !out) return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_create: cfg/out is NULL");
    *out = nullptr;
    if (h->P.policy_a != nullptr || h->P.policy_b != nullptr)
        return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_create needs a two-player handle: neither side may have a fixed policy (soccer_set_policy)");
    if (!(h->cfg.flags & SOCCER_F_AUTORESET))
        return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_create needs a handle created with SOCCER_F_AUTORESET");
    if (h->cfg.n_lanes > SOCCER_MQ_MAX_LANES)
        return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_create: more than 2^22 lanes (%llu): the integer sums of a step could overflow",
                    (unsigned long long)h->cfg.n_lanes);
    if (!(cfg->discount_factor >= 0.0 && cfg->discount_factor < 1.0)) return fail(h, SOCCER_E_INVALID, "discount_factor must be in [0, 1)");
    if (!(cfg->alpha >= 0.0 && cfg->alpha <= 1.0)) return fail(h, SOCCER_E_INVALID, "alpha must be in [0, 1]");
    if (!(cfg->decay > 0.0 && cfg->decay <= 1.0)) return fail(h, SOCCER_E_INVALID, "decay must be in (0, 1]");
    if (!(cfg->explor >= 0.0 && cfg->explor <= 1.0)) return fail(h, SOCCER_E_INVALID, "explor must be in [0, 1]");
    if (!(cfg->q_init >= -1.0 && cfg->q_init <= 1.0)) return fail(h, SOCCER_E_INVALID, "q_init must be in [-1, 1]");
    if (cfg->opponent != SOCCER_MQ_UNIFORM && cfg->opponent != SOCCER_MQ_SELF && cfg->opponent != SOCCER_MQ_FIXED)
        return fail(h, SOCCER_E_INVALID, "opponent must be SOCCER_MQ_UNIFORM, SOCCER_MQ_SELF or SOCCER_MQ_FIXED");
    if ((cfg->opponent == SOCCER_MQ_FIXED) != (cfg->opponent_policy != nullptr))
        return fail(h, SOCCER_E_INVALID, "opponent_policy goes with SOCCER_MQ_FIXED, and only with it");
    const int nS = h->rules.nS;
    std::vector<uint16_t> fixed;
    if (cfg->opponent == SOCCER_MQ_FIXED)
        if (int rc = fixed_thresholds(h, "opponent_policy", cfg->opponent_policy, nS, fixed)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, act(h, h->P, LearnerIO{}));                   // (an empty block: the LDS limit of this handle's act kernel, nothing launched)
    std::unique_ptr<soccer_minimax_q> owner(new soccer_minimax_q());
    soccer_minimax_q* q = owner.get();
    q->h = h;
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
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // `fixed` is pageable host memory of this call
    h->learners.push_back(q);
    *out = owner.release();
    return SOCCER_OK;
}

extern "C" int soccer_minimax_q_destroy(soccer_handle* h, soccer_minimax_q* q) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (!q) return SOCCER_OK;
    if (int rc = learner_check(h, q, "soccer_minimax_q_destroy")) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // nothing is freed under a kernel that reads it
    h->learners.erase(std::find(h->learners.begin(), h->learners.end(), q));
    delete q;
    return SOCCER_OK;
}

extern "C" int soccer_minimax_q_run(soccer_handle* h, soccer_minimax_q* q, int32_t n_steps) {
    if (int rc = learner_check(h, q, "soccer_minimax_q_run")) return rc;
    if (n_steps < 0) return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_run: n_steps must be >= 0");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    for (int32_t t = 0; t < n_steps; ++t) {
        KernelParams P = h->P;
        bind_tick(h, P, 1);
        HIP_TRY(h, act(h, P, q->io));
        launch_update(q);
    }
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

extern "C" int soccer_minimax_q_update(soccer_handle* h, soccer_minimax_q* q, int64_t n, const uint16_t* obs, const int8_t* act_a,
                                       const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs) {
    if (int rc = learner_check(h, q, "soccer_minimax_q_update")) return rc;
    if (n < 0 || n > (int64_t)SOCCER_MQ_MAX_LANES) return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_update: n must be in 0..2^22");
    if (n > 0 && (!obs || !act_a || !act_b || !reward || !terminated || !next_obs))
        return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_update: all six transition arrays are required");
    if (!aligned(obs, 2) || !aligned(next_obs, 2)) return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_update: obs / next_obs must be 2-byte aligned");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (n > 0)
        hipLaunchKernelGGL(learner_reduce_kernel, dim3(grid_for(h, (uint64_t)n)), dim3(kBlock), 0, h->stream, q->io, (long long)n,
                           obs, act_a, act_b, reward, terminated, next_obs);
    launch_update(q);
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

extern "C" int soccer_minimax_q_read(soccer_handle* h, soccer_minimax_q* q, double* Q, double* V, double* pi_a, double* pi_b,
                                     uint64_t* visits, double* alpha, uint64_t* steps) {
    if (int rc = learner_check(h, q, "soccer_minimax_q_read")) return rc;
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
    if (int rc = learner_check(h, q, "soccer_minimax_q_load")) return rc;
    if (!Q) return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_load: Q is NULL");
    const LearnerIO& io = q->io;
    const size_t nS = (size_t)io.nS;
    for (size_t i = 25; i < nS * 25; ++i)
        if (!(Q[i] >= -1.0 && Q[i] <= 1.0)) return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_load: Q[%zu][%zu][%zu] is outside [-1, 1]", i / 25, i % 25 / 5, i % 5);
    if (alpha && !(*alpha >= 0.0 && *alpha <= 1.0)) return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_load: alpha must be in [0, 1]");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipMemsetAsync(io.Q, 0, 200, h->stream));                          // Q[0] = 0
    HIP_TRY(h, hipMemcpyAsync(io.Q + 25, Q + 25, (nS - 1) * 200, hipMemcpyHostToDevice, h->stream));
    if (visits) HIP_TRY(h, hipMemcpyAsync(io.visits, visits, nS * 200, hipMemcpyHostToDevice, h->stream));
    if (alpha) HIP_TRY(h, hipMemcpyAsync(io.alpha + q->slot, alpha, 8, hipMemcpyHostToDevice, h->stream));
    if (steps) HIP_TRY(h, hipMemcpyAsync(io.steps, steps, 8, hipMemcpyHostToDevice, h->stream));
    const unsigned grid = (unsigned)((io.nS + kLearnerWaves - 1) / kLearnerWaves);
    if (visits) hipLaunchKernelGGL(learner_update_kernel<1>, dim3(grid), dim3(kLearnerBlock), 0, h->stream, io, q->slot);
    else hipLaunchKernelGGL(learner_update_kernel<2>, dim3(grid), dim3(kLearnerBlock), 0, h->stream, io, q->slot);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // the caller's arrays are pageable host memory
    return SOCCER_OK;
}

// =================================================================================================
// independent Q-learners: soccer_q_learner_*
// =================================================================================================
static int q_check(soccer_handle* h, soccer_q_learner* q, const char* what) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "%s during graph capture", what);
    if (!q || std::find(h->q_learners.begin(), h->q_learners.end(), q) == h->q_learners.end())
        return fail(h, SOCCER_E_INVALID, "%s: not a learner of this handle", what);
    return SOCCER_OK;
}

template <bool SLIP, bool LUT_LDS>
static hipError_t launch_q_act(soccer_handle* h, const KernelParams& P, const QLearnerIO& io) {
    if (io.nS == 0)                     // soccer_q_learner_create: the LDS limit, as launch_act
        return h->smem_bytes > 48 * 1024 ? hipFuncSetAttribute(reinterpret_cast<const void*>(&q_act_kernel<SLIP, LUT_LDS>),
                                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->smem_bytes) : hipSuccess;
    hipLaunchKernelGGL((q_act_kernel<SLIP, LUT_LDS>), dim3(grid_for(h, P.n)), dim3(kBlock), h->smem_bytes, h->stream, P, io);
    return hipSuccess;
}

static hipError_t q_act(soccer_handle* h, const KernelParams& P, const QLearnerIO& io) {
    return h->slip ? (h->lut_lds ? launch_q_act<true, true>(h, P, io) : launch_q_act<true, false>(h, P, io))
                   : (h->lut_lds ? launch_q_act<false, true>(h, P, io) : launch_q_act<false, false>(h, P, io));
}

static unsigned q_update_grid(const QLearnerIO& io) { return (unsigned)((io.nS + kQStates - 1) / kQStates); }

static void launch_q_update(soccer_q_learner* q) {
    hipLaunchKernelGGL(q_update_kernel<0>, dim3(q_update_grid(q->io)), dim3(kLearnerBlock), 0, q->h->stream, q->io, q->slot);
    q->slot ^= 1;
}

static bool ql_kind(int32_t k) { return k == SOCCER_QL_GREEDY || k == SOCCER_QL_UNIFORM || k == SOCCER_QL_FIXED; }

extern "C" int soccer_q_learner_create(soccer_handle* h, const soccer_q_learner_config* cfg, soccer_q_learner** out) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_q_learner_create during graph capture");
    if (!cfg || !out) return fail(h, SOCCER_E_INVALID, "soccer_q_learner_create: cfg/out is NULL");
    *out = nullptr;
    if (h->P.policy_a != nullptr || h->P.policy_b != nullptr)
        return fail(h, SOCCER_E_INVALID, "soccer_q_learner_create needs a two-player handle: neither side may have a fixed policy (soccer_set_policy)");
    if (!(h->cfg.flags & SOCCER_F_AUTORESET))
        return fail(h, SOCCER_E_INVALID, "soccer_q_learner_create needs a handle created with SOCCER_F_AUTORESET");
    if (h->cfg.n_lanes > SOCCER_MQ_MAX_LANES)
        return fail(h, SOCCER_E_INVALID, "soccer_q_learner_create: more than 2^22 lanes (%llu): the integer sums of a step could overflow",
                    (unsigned long long)h->cfg.n_lanes);
    if (!(cfg->discount_factor >= 0.0 && cfg->discount_factor < 1.0)) return fail(h, SOCCER_E_INVALID, "discount_factor must be in [0, 1)");
    if (!(cfg->alpha >= 0.0 && cfg->alpha <= 1.0)) return fail(h, SOCCER_E_INVALID, "alpha must be in [0, 1]");
    if (!(cfg->decay > 0.0 && cfg->decay <= 1.0)) return fail(h, SOCCER_E_INVALID, "decay must be in (0, 1]");
    if (!(cfg->explor >= 0.0 && cfg->explor <= 1.0)) return fail(h, SOCCER_E_INVALID, "explor must be in [0, 1]");
    if (!(cfg->q_init >= -1.0 && cfg->q_init <= 1.0)) return fail(h, SOCCER_E_INVALID, "q_init must be in [-1, 1]");
    if (!ql_kind(cfg->act_a) || !ql_kind(cfg->act_b))
        return fail(h, SOCCER_E_INVALID, "act_a / act_b must be SOCCER_QL_GREEDY, SOCCER_QL_UNIFORM or SOCCER_QL_FIXED");
    if ((cfg->act_a == SOCCER_QL_FIXED) != (cfg->policy_a != nullptr)) return fail(h, SOCCER_E_INVALID, "policy_a goes with act_a == SOCCER_QL_FIXED, and only with it");
    if ((cfg->act_b == SOCCER_QL_FIXED) != (cfg->policy_b != nullptr)) return fail(h, SOCCER_E_INVALID, "policy_b goes with act_b == SOCCER_QL_FIXED, and only with it");
    const int nS = h->rules.nS;
    std::vector<uint16_t> fixed[2];
    if (cfg->policy_a) if (int rc = fixed_thresholds(h, "policy_a", cfg->policy_a, nS, fixed[0])) return rc;
    if (cfg->policy_b) if (int rc = fixed_thresholds(h, "policy_b", cfg->policy_b, nS, fixed[1])) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, q_act(h, h->P, QLearnerIO{}));                // (an empty block: the LDS limit of this handle's act kernel, nothing launched)
    std::unique_ptr<soccer_q_learner> owner(new soccer_q_learner());
    soccer_q_learner* q = owner.get();
    q->h = h;
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
    hipLaunchKernelGGL(q_update_kernel<1>, dim3(q_update_grid(io)), dim3(kLearnerBlock), 0, h->stream, io, 0);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // `fixed` is pageable host memory of this call
    h->q_learners.push_back(q);
    *out = owner.release();
    return SOCCER_OK;
}

extern "C" int soccer_q_learner_destroy(soccer_handle* h, soccer_q_learner* q) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (!q) return SOCCER_OK;
    if (int rc = q_check(h, q, "soccer_q_learner_destroy")) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // nothing is freed under a kernel that reads it
    h->q_learners.erase(std::find(h->q_learners.begin(), h->q_learners.end(), q));
    delete q;
    return SOCCER_OK;
}

extern "C" int soccer_q_learner_run(soccer_handle* h, soccer_q_learner* q, int32_t n_steps) {
    if (int rc = q_check(h, q, "soccer_q_learner_run")) return rc;
    if (n_steps < 0) return fail(h, SOCCER_E_INVALID, "soccer_q_learner_run: n_steps must be >= 0");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    for (int32_t t = 0; t < n_steps; ++t) {
        KernelParams P = h->P;
        bind_tick(h, P, 1);
        HIP_TRY(h, q_act(h, P, q->io));
        launch_q_update(q);
    }
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

extern "C" int soccer_q_learner_update(soccer_handle* h, soccer_q_learner* q, int64_t n, const uint16_t* obs, const int8_t* act_a,
                                       const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs) {
    if (int rc = q_check(h, q, "soccer_q_learner_update")) return rc;
    if (n < 0 || n > (int64_t)SOCCER_MQ_MAX_LANES) return fail(h, SOCCER_E_INVALID, "soccer_q_learner_update: n must be in 0..2^22");
    if (n > 0 && (!obs || !act_a || !act_b || !reward || !terminated || !next_obs))
        return fail(h, SOCCER_E_INVALID, "soccer_q_learner_update: all six transition arrays are required");
    if (!aligned(obs, 2) || !aligned(next_obs, 2)) return fail(h, SOCCER_E_INVALID, "soccer_q_learner_update: obs / next_obs must be 2-byte aligned");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (n > 0)
        hipLaunchKernelGGL(q_reduce_kernel, dim3(grid_for(h, (uint64_t)n)), dim3(kBlock), 0, h->stream, q->io, (long long)n,
                           obs, act_a, act_b, reward, terminated, next_obs);
    launch_q_update(q);
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

extern "C" int soccer_q_learner_read(soccer_handle* h, soccer_q_learner* q, double* Q_a, double* Q_b, uint64_t* visits,
                                     double* alpha, uint64_t* steps) {
    if (int rc = q_check(h, q, "soccer_q_learner_read")) return rc;
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
    if (int rc = q_check(h, q, "soccer_q_learner_load")) return rc;
    if (!Q_a || !Q_b) return fail(h, SOCCER_E_INVALID, "soccer_q_learner_load: Q_a / Q_b is NULL");
    const QLearnerIO& io = q->io;
    const size_t nS = (size_t)io.nS;
    const double* Q[2] = {Q_a, Q_b};
    for (int p = 0; p < 2; ++p)
        for (size_t i = 5; i < nS * 5; ++i)
            if (!(Q[p][i] >= -1.0 && Q[p][i] <= 1.0))
                return fail(h, SOCCER_E_INVALID, "soccer_q_learner_load: Q_%c[%zu][%zu] is outside [-1, 1]", p ? 'b' : 'a', i / 5, i % 5);
    if (alpha && !(*alpha >= 0.0 && *alpha <= 1.0)) return fail(h, SOCCER_E_INVALID, "soccer_q_learner_load: alpha must be in [0, 1]");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    for (int p = 0; p < 2; ++p) {
        HIP_TRY(h, hipMemsetAsync(io.Q[p], 0, 40, h->stream));                    // Q_p[0] = 0
        HIP_TRY(h, hipMemcpyAsync(io.Q[p] + 5, Q[p] + 5, (nS - 1) * 40, hipMemcpyHostToDevice, h->stream));
    }
    if (visits) HIP_TRY(h, hipMemcpyAsync(io.visits, visits, nS * 200, hipMemcpyHostToDevice, h->stream));
    else HIP_TRY(h, hipMemsetAsync(io.visits, 0, nS * 200, h->stream));
    if (alpha) HIP_TRY(h, hipMemcpyAsync(io.alpha + q->slot, alpha, 8, hipMemcpyHostToDevice, h->stream));
    if (steps) HIP_TRY(h, hipMemcpyAsync(io.steps, steps, 8, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(q_update_kernel<1>, dim3(q_update_grid(io)), dim3(kLearnerBlock), 0, h->stream, io, q->slot);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // the caller's arrays are pageable host memory
    return SOCCER_OK;
}

// =================================================================================================
// policy hill-climbers: soccer_wolf_phc_*
// =================================================================================================
static int phc_check(soccer_handle* h, soccer_wolf_phc* q, const char* what) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "%s during graph capture", what);
    if (!q || std::find(h->phc_learners.begin(), h->phc_learners.end(), q) == h->phc_learners.end())
        return fail(h, SOCCER_E_INVALID, "%s: not a learner of this handle", what);
    return SOCCER_OK;
}

template <bool SLIP, bool LUT_LDS>
static hipError_t launch_phc_act(soccer_handle* h, const KernelParams& P, const PhcIO& io) {
    if (io.nS == 0)                     // soccer_wolf_phc_create: the LDS limit, as launch_act
        return h->smem_bytes > 48 * 1024 ? hipFuncSetAttribute(reinterpret_cast<const void*>(&phc_act_kernel<SLIP, LUT_LDS>),
                                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->smem_bytes) : hipSuccess;
    hipLaunchKernelGGL((phc_act_kernel<SLIP, LUT_LDS>), dim3(grid_for(h, P.n)), dim3(kBlock), h->smem_bytes, h->stream, P, io);
    return hipSuccess;
}

static hipError_t phc_act(soccer_handle* h, const KernelParams& P, const PhcIO& io) {
    return h->slip ? (h->lut_lds ? launch_phc_act<true, true>(h, P, io) : launch_phc_act<true, false>(h, P, io))
                   : (h->lut_lds ? launch_phc_act<false, true>(h, P, io) : launch_phc_act<false, false>(h, P, io));
}

static void launch_phc_update(soccer_wolf_phc* q) {
    hipLaunchKernelGGL(phc_update_kernel<0>, dim3(q_update_grid(q->io)), dim3(kLearnerBlock), 0, q->h->stream, q->io, q->slot);
    q->slot ^= 1;
}

static bool phc_kind(int32_t k) { return k == SOCCER_PHC_LEARN || k == SOCCER_PHC_UNIFORM || k == SOCCER_PHC_FIXED; }

// rows 1.. of a checkpoint's policy array, held to what fixed_thresholds holds a fixed policy to
static int policy_rows_check(soccer_handle* h, const char* name, const double* policy, int nS) {
    for (int s = 1; s < nS; ++s) {
        const double* p = policy + (size_t)s * 5;
        double sum = 0.0;
        for (int k = 0; k < 5; ++k) {
            if (!(p[k] >= 0.0)) return fail(h, SOCCER_E_INVALID, "soccer_wolf_phc_load: %s[%d][%d] is negative or not a number", name, s, k);
            sum = sum + p[k];
        }
        if (!(std::fabs(sum - 1.0) <= 1e-8 + 1e-5)) return fail(h, SOCCER_E_INVALID, "soccer_wolf_phc_load: %s[%d] does not sum to 1", name, s);
    }
    return SOCCER_OK;
}

extern "C" int soccer_wolf_phc_create(soccer_handle* h, const soccer_wolf_phc_config* cfg, soccer_wolf_phc** out) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_wolf_phc_create during graph capture");
    if (!cfg || !out) return fail(h, SOCCER_E_INVALID, "soccer_wolf_phc_create: cfg/out is NULL");
    *out = nullptr;
    if (h->P.policy_a != nullptr || h->P.policy_b != nullptr)
        return fail(h, SOCCER_E_INVALID, "soccer_wolf_phc_create needs a two-player handle: neither side may have a fixed policy (soccer_set_policy)");
    if (!(h->cfg.flags & SOCCER_F_AUTORESET))
        return fail(h, SOCCER_E_INVALID, "soccer_wolf_phc_create needs a handle created with SOCCER_F_AUTORESET");
    if (h->cfg.n_lanes > SOCCER_MQ_MAX_LANES)
        return fail(h, SOCCER_E_INVALID, "soccer_wolf_phc_create: more than 2^22 lanes (%llu): the integer sums of a step could overflow",
                    (unsigned long long)h->cfg.n_lanes);
    if (!(cfg->discount_factor >= 0.0 && cfg->discount_factor < 1.0)) return fail(h, SOCCER_E_INVALID, "discount_factor must be in [0, 1)");
    if (!(cfg->alpha >= 0.0 && cfg->alpha <= 1.0)) return fail(h, SOCCER_E_INVALID, "alpha must be in [0, 1]");
    if (!(cfg->decay > 0.0 && cfg->decay <= 1.0)) return fail(h, SOCCER_E_INVALID, "decay must be in (0, 1]");
    if (!(cfg->explor >= 0.0 && cfg->explor <= 1.0)) return fail(h, SOCCER_E_INVALID, "explor must be in [0, 1]");
    if (!(cfg->q_init >= -1.0 && cfg->q_init <= 1.0)) return fail(h, SOCCER_E_INVALID, "q_init must be in [-1, 1]");
    if (!(cfg->delta_win >= 0.0 && cfg->delta_win <= 1.0)) return fail(h, SOCCER_E_INVALID, "delta_win must be in [0, 1]");
    if (!(cfg->delta_lose >= 0.0 && cfg->delta_lose <= 1.0)) return fail(h, SOCCER_E_INVALID, "delta_lose must be in [0, 1]");
    if (!(cfg->delta_decay > 0.0 && cfg->delta_decay <= 1.0)) return fail(h, SOCCER_E_INVALID, "delta_decay must be in (0, 1]");
    if (!phc_kind(cfg->act_a) || !phc_kind(cfg->act_b))
        return fail(h, SOCCER_E_INVALID, "act_a / act_b must be SOCCER_PHC_LEARN, SOCCER_PHC_UNIFORM or SOCCER_PHC_FIXED");
    if ((cfg->act_a == SOCCER_PHC_FIXED) != (cfg->policy_a != nullptr)) return fail(h, SOCCER_E_INVALID, "policy_a goes with act_a == SOCCER_PHC_FIXED, and only with it");
    if ((cfg->act_b == SOCCER_PHC_FIXED) != (cfg->policy_b != nullptr)) return fail(h, SOCCER_E_INVALID, "policy_b goes with act_b == SOCCER_PHC_FIXED, and only with it");
    const int nS = h->rules.nS;
    const int32_t kinds[2] = {cfg->act_a, cfg->act_b};
    const double* policy[2] = {cfg->policy_a, cfg->policy_b};
    std::vector<uint16_t> fixed[2];
    if (cfg->policy_a) if (int rc = fixed_thresholds(h, "policy_a", cfg->policy_a, nS, fixed[0])) return rc;
    if (cfg->policy_b) if (int rc = fixed_thresholds(h, "policy_b", cfg->policy_b, nS, fixed[1])) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, phc_act(h, h->P, PhcIO{}));                   // (an empty block: the LDS limit of this handle's act kernel, nothing launched)
    std::unique_ptr<soccer_wolf_phc> owner(new soccer_wolf_phc());
    soccer_wolf_phc* q = owner.get();
    q->h = h;
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
    hipLaunchKernelGGL(phc_update_kernel<1>, dim3(q_update_grid(io)), dim3(kLearnerBlock), 0, h->stream, io, 0);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // `fixed` and the policies are pageable host memory of this call
    h->phc_learners.push_back(q);
    *out = owner.release();
    return SOCCER_OK;
}

extern "C" int soccer_wolf_phc_destroy(soccer_handle* h, soccer_wolf_phc* q) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (!q) return SOCCER_OK;
    if (int rc = phc_check(h, q, "soccer_wolf_phc_destroy")) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // nothing is freed under a kernel that reads it
    h->phc_learners.erase(std::find(h->phc_learners.begin(), h->phc_learners.end(), q));
    delete q;
    return SOCCER_OK;
}

extern "C" int soccer_wolf_phc_run(soccer_handle* h, soccer_wolf_phc* q, int32_t n_steps) {
    if (int rc = phc_check(h, q, "soccer_wolf_phc_run")) return rc;
    if (n_steps < 0) return fail(h, SOCCER_E_INVALID, "soccer_wolf_phc_run: n_steps must be >= 0");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    for (int32_t t = 0; t < n_steps; ++t) {
        KernelParams P = h->P;
        bind_tick(h, P, 1);
        HIP_TRY(h, phc_act(h, P, q->io));
        launch_phc_update(q);
    }
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

extern "C" int soccer_wolf_phc_update(soccer_handle* h, soccer_wolf_phc* q, int64_t n, const uint16_t* obs, const int8_t* act_a,
                                      const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs) {
    if (int rc = phc_check(h, q, "soccer_wolf_phc_update")) return rc;
    if (n < 0 || n > (int64_t)SOCCER_MQ_MAX_LANES) return fail(h, SOCCER_E_INVALID, "soccer_wolf_phc_update: n must be in 0..2^22");
    if (n > 0 && (!obs || !act_a || !act_b || !reward || !terminated || !next_obs))
        return fail(h, SOCCER_E_INVALID, "soccer_wolf_phc_update: all six transition arrays are required");
    if (!aligned(obs, 2) || !aligned(next_obs, 2)) return fail(h, SOCCER_E_INVALID, "soccer_wolf_phc_update: obs / next_obs must be 2-byte aligned");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (n > 0)
        hipLaunchKernelGGL(phc_reduce_kernel, dim3(grid_for(h, (uint64_t)n)), dim3(kBlock), 0, h->stream, q->io, (long long)n,
                           obs, act_a, act_b, reward, terminated, next_obs);
    launch_phc_update(q);
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

extern "C" int soccer_wolf_phc_read(soccer_handle* h, soccer_wolf_phc* q, const soccer_wolf_phc_state* out) {
    if (int rc = phc_check(h, q, "soccer_wolf_phc_read")) return rc;
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
    if (int rc = phc_check(h, q, "soccer_wolf_phc_load")) return rc;
    if (!in || !in->Q_a || !in->Q_b) return fail(h, SOCCER_E_INVALID, "soccer_wolf_phc_load: in / Q_a / Q_b is NULL");
    const PhcIO& io = q->io;
    const size_t nS = (size_t)io.nS;
    const double* Q[2] = {in->Q_a, in->Q_b};
    // a player that does not LEARN keeps its constant rows
    const double* rows[4] = {io.learn[0] ? in->pi_a : nullptr, io.learn[1] ? in->pi_b : nullptr,
                             io.learn[0] ? in->avg_a : nullptr, io.learn[1] ? in->avg_b : nullptr};
    double* const to[4] = {io.pi[0], io.pi[1], io.avg[0], io.avg[1]};
    static const char* const names[4] = {"pi_a", "pi_b", "avg_a", "avg_b"};
    for (int p = 0; p < 2; ++p)
        for (size_t i = 5; i < nS * 5; ++i)
            if (!(Q[p][i] >= -1.0 && Q[p][i] <= 1.0))
                return fail(h, SOCCER_E_INVALID, "soccer_wolf_phc_load: Q_%c[%zu][%zu] is outside [-1, 1]", p ? 'b' : 'a', i / 5, i % 5);
    for (int i = 0; i < 4; ++i)
        if (rows[i]) if (int rc = policy_rows_check(h, names[i], rows[i], io.nS)) return rc;
    if (in->alpha && !(*in->alpha >= 0.0 && *in->alpha <= 1.0)) return fail(h, SOCCER_E_INVALID, "soccer_wolf_phc_load: alpha must be in [0, 1]");
    if (in->dscale && !(*in->dscale >= 0.0 && *in->dscale <= 1.0)) return fail(h, SOCCER_E_INVALID, "soccer_wolf_phc_load: dscale must be in [0, 1]");
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
    hipLaunchKernelGGL(phc_update_kernel<1>, dim3(q_update_grid(io)), dim3(kLearnerBlock), 0, h->stream, io, q->slot);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // the caller's arrays are pageable host memory
    return SOCCER_OK;
}

// =================================================================================================
// populations of independent Q-learners, a learner per lane: soccer_q_population_*
// =================================================================================================
static_assert(kPopGreedy == SOCCER_QL_GREEDY && kPopUniform == SOCCER_QL_UNIFORM, "the kernels' names of the modes");

static int pop_check(soccer_handle* h, soccer_q_population* q, const char* what) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "%s during graph capture", what);
    if (!q || std::find(h->q_populations.begin(), h->q_populations.end(), q) == h->q_populations.end())
        return fail(h, SOCCER_E_INVALID, "%s: not a population of this handle", what);
    return SOCCER_OK;
}

static int pop_range_check(soccer_handle* h, const soccer_q_population* q, const char* what, int64_t first, int64_t count) {
    if (first < 0 || count < 0 || (uint64_t)first > q->n || (uint64_t)count > q->n - (uint64_t)first)
        return fail(h, SOCCER_E_INVALID, "%s: members %lld .. %lld + %lld are outside the population of %llu", what, (long long)first,
                    (long long)first, (long long)count, q->n);
    return SOCCER_OK;
}

// SOCCER_POP_GRID_BLOCKS, read at creation (tests: a grid-stride loop over members that wraps on a small population, as
// SOCCER_MQ_POP_WAVES does for the minimax-Q population): 1 .. the handle's grid_cap, ignored otherwise
static int pop_grid_blocks_env(const soccer_handle* h) {
    if (const char* e = std::getenv("SOCCER_POP_GRID_BLOCKS")) {
        const long v = std::atol(e);
        if (v >= 1 && v <= (long)h->grid_cap) return (int)v;
    }
    return 0;
}

// the grid of a population's run / update launch: grid_for, under the population's own cap where it has one
static int pop_grid(const soccer_handle* h, int grid_blocks, uint64_t members) {
    const int g = grid_for(h, members);
    return grid_blocks > 0 && g > grid_blocks ? grid_blocks : g;
}

// launch == false (soccer_q_population_create): the LDS limit of this handle's run kernel, as launch_act
template <bool SLIP, bool LUT_LDS>
static hipError_t launch_pop_run(soccer_handle* h, const KernelParams& P, const PopIO& io, bool launch, int grid_blocks) {
    if (!launch)
        return h->smem_bytes > 48 * 1024 ? hipFuncSetAttribute(reinterpret_cast<const void*>(&pop_run_kernel<SLIP, LUT_LDS>),
                                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->smem_bytes) : hipSuccess;
    hipLaunchKernelGGL((pop_run_kernel<SLIP, LUT_LDS>), dim3(pop_grid(h, grid_blocks, P.n)), dim3(kBlock), h->smem_bytes, h->stream, P, io);
    return hipSuccess;
}

static hipError_t pop_run(soccer_handle* h, const KernelParams& P, const PopIO& io, bool launch, int grid_blocks = 0) {
    return h->slip ? (h->lut_lds ? launch_pop_run<true, true>(h, P, io, launch, grid_blocks) : launch_pop_run<true, false>(h, P, io, launch, grid_blocks))
                   : (h->lut_lds ? launch_pop_run<false, true>(h, P, io, launch, grid_blocks) : launch_pop_run<false, false>(h, P, io, launch, grid_blocks));
}

// the same for a population with a league opponent
template <bool SLIP, bool LUT_LDS>
static hipError_t launch_pop_league_run(soccer_handle* h, const KernelParams& P, const PopIO& io, const PopLeagueIO& lg, bool launch, int grid_blocks) {
    if (!launch)
        return h->smem_bytes > 48 * 1024 ? hipFuncSetAttribute(reinterpret_cast<const void*>(&pop_league_run_kernel<SLIP, LUT_LDS>),
                                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->smem_bytes) : hipSuccess;
    hipLaunchKernelGGL((pop_league_run_kernel<SLIP, LUT_LDS>), dim3(pop_grid(h, grid_blocks, P.n)), dim3(kBlock), h->smem_bytes, h->stream, P, io, lg);
    return hipSuccess;
}

static hipError_t pop_league_run(soccer_handle* h, const KernelParams& P, const PopIO& io, const PopLeagueIO& lg, bool launch, int grid_blocks = 0) {
    return h->slip ? (h->lut_lds ? launch_pop_league_run<true, true>(h, P, io, lg, launch, grid_blocks) : launch_pop_league_run<true, false>(h, P, io, lg, launch, grid_blocks))
                   : (h->lut_lds ? launch_pop_league_run<false, true>(h, P, io, lg, launch, grid_blocks) : launch_pop_league_run<false, false>(h, P, io, lg, launch, grid_blocks));
}

// a hyperparameter of every member: the caller's n values, each held to the scalar's range, or the scalar n times
template <class Ok>
static int pop_param(soccer_handle* h, const char* name, const char* range, const double* per_member, double scalar, size_t n, Ok ok,
                     std::vector<double>& out) {
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

// what soccer_q_population_create_league adds to a creation: the league's player, its K policies and their weights (HOST)
struct PopLeagueSpec {
    int32_t player, K;
    const double* policies;             // [K][nS][5]
    const double* weights;              // [K]
};

// both creations; `what` names the entry point in the messages, lg == nullptr: no league
static int pop_create(soccer_handle* h, const soccer_q_population_config* cfg, const PopLeagueSpec* lg, const char* what,
                      soccer_q_population** out) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "%s during graph capture", what);
    if (!cfg || !out) return fail(h, SOCCER_E_INVALID, "%s: cfg/out is NULL", what);
    *out = nullptr;
    if (h->P.policy_a != nullptr || h->P.policy_b != nullptr)
        return fail(h, SOCCER_E_INVALID, "%s needs a two-player handle: neither side may have a fixed policy (soccer_set_policy)", what);
    if (!(h->cfg.flags & SOCCER_F_AUTORESET))
        return fail(h, SOCCER_E_INVALID, "%s needs a handle created with SOCCER_F_AUTORESET", what);
    const size_t n = (size_t)h->cfg.n_lanes;
    std::vector<double> par[4];         // alpha, decay, explor, discount_factor
    if (int rc = pop_param(h, "discount_factor", "[0, 1)", cfg->discount_factor_per_member, cfg->discount_factor, n,
                           [](double x) { return x >= 0.0 && x < 1.0; }, par[3])) return rc;
    if (int rc = pop_param(h, "alpha", "[0, 1]", cfg->alpha_per_member, cfg->alpha, n, [](double x) { return x >= 0.0 && x <= 1.0; }, par[0])) return rc;
    if (int rc = pop_param(h, "decay", "(0, 1]", cfg->decay_per_member, cfg->decay, n, [](double x) { return x > 0.0 && x <= 1.0; }, par[1])) return rc;
    if (int rc = pop_param(h, "explor", "[0, 1]", cfg->explor_per_member, cfg->explor, n, [](double x) { return x >= 0.0 && x <= 1.0; }, par[2])) return rc;
    if (!(cfg->q_init >= -1.0 && cfg->q_init <= 1.0)) return fail(h, SOCCER_E_INVALID, "q_init must be in [-1, 1]");
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
    if (cfg->policy_a) if (int rc = fixed_thresholds(h, "policy_a", cfg->policy_a, nS, fixed[0])) return rc;
    if (cfg->policy_b) if (int rc = fixed_thresholds(h, "policy_b", cfg->policy_b, nS, fixed[1])) return rc;
    std::vector<uint16_t> league_thr;   // [K][nS][4]
    std::vector<uint64_t> league_T;     // [K - 1]
    if (lg) {
        const int bad = league_check_weights(lg->weights, lg->K);
        if (bad >= 0 && bad < lg->K) return fail(h, SOCCER_E_INVALID, "weights[%d] is negative or not a finite number", bad);
        if (bad == lg->K) return fail(h, SOCCER_E_INVALID, "weights does not sum to 1");
        league_thr.reserve((size_t)lg->K * (size_t)nS * 4);
        std::vector<uint16_t> one;
        char name[48];
        for (int k = 0; k < lg->K; ++k) {
            std::snprintf(name, sizeof name, "policies[%d]", k);
            if (int rc = fixed_thresholds(h, name, lg->policies + (size_t)k * (size_t)nS * 5, nS, one)) return rc;
            league_thr.insert(league_thr.end(), one.begin(), one.end());
        }
        league_T.assign((size_t)std::max(lg->K - 1, 1), 0);        // (K == 1: one unread entry, so that no pointer is NULL)
        league_thresholds(lg->weights, lg->K, league_T.data());
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, lg ? pop_league_run(h, h->P, PopIO{}, PopLeagueIO{}, false) : pop_run(h, h->P, PopIO{}, false));
    std::unique_ptr<soccer_q_population> owner(new soccer_q_population());
    soccer_q_population* q = owner.get();
    q->h = h; q->n = n;
    if (const char* e = std::getenv("SOCCER_POP_LAUNCH_STEPS")) {      // (tests: a launch boundary within a short run)
        const long v = std::atol(e);
        if (v >= 1 && v <= 4096) q->launch_steps = (int)v;
    }
    q->grid_blocks = pop_grid_blocks_env(h);
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
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // the vectors are pageable host memory of this call
    h->q_populations.push_back(q);
    *out = owner.release();
    return SOCCER_OK;
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
    if (int rc = pop_check(h, q, what)) return rc;
    if (q->league.K == 0) return fail(h, SOCCER_E_INVALID, "%s: this population has no league (soccer_q_population_create_league)", what);
    return pop_range_check(h, q, what, first, count);
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

extern "C" int soccer_q_population_destroy(soccer_handle* h, soccer_q_population* q) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (!q) return SOCCER_OK;
    if (int rc = pop_check(h, q, "soccer_q_population_destroy")) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // nothing is freed under a kernel that reads it
    h->q_populations.erase(std::find(h->q_populations.begin(), h->q_populations.end(), q));
    delete q;
    return SOCCER_OK;
}

extern "C" int soccer_q_population_run(soccer_handle* h, soccer_q_population* q, int32_t n_steps) {
    if (int rc = pop_check(h, q, "soccer_q_population_run")) return rc;
    if (n_steps < 0) return fail(h, SOCCER_E_INVALID, "soccer_q_population_run: n_steps must be >= 0");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    // the tick sequence of consecutive launches is contiguous and a member's whole state is in memory between them, so the
    // split changes no result
    // (a league's kick-off draws take the blocks of counter 2^62 + tick: below 2^62 a tick's own blocks are never met)
    if (q->league.K != 0 && (h->tick >= (1ull << 62) || (uint64_t)n_steps > (1ull << 62) - h->tick))
        return fail(h, SOCCER_E_INVALID, "soccer_q_population_run: a league population's run may not cross tick 2^62");
    for (int32_t t0 = 0; t0 < n_steps; t0 += q->launch_steps) {
        KernelParams P = h->P;
        PopIO io = q->io;
        io.n_steps = n_steps - t0 < q->launch_steps ? n_steps - t0 : q->launch_steps;
        bind_tick(h, P, (uint64_t)io.n_steps);
        HIP_TRY(h, q->league.K != 0 ? pop_league_run(h, P, io, q->league, true, q->grid_blocks) : pop_run(h, P, io, true, q->grid_blocks));
    }
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

extern "C" int soccer_q_population_update(soccer_handle* h, soccer_q_population* q, const uint16_t* obs, const int8_t* act_a,
                                          const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs) {
    if (int rc = pop_check(h, q, "soccer_q_population_update")) return rc;
    if (!obs || !act_a || !act_b || !reward || !terminated || !next_obs)
        return fail(h, SOCCER_E_INVALID, "soccer_q_population_update: all six transition arrays are required");
    if (!aligned(obs, 2) || !aligned(next_obs, 2)) return fail(h, SOCCER_E_INVALID, "soccer_q_population_update: obs / next_obs must be 2-byte aligned");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipLaunchKernelGGL(pop_update_kernel, dim3(pop_grid(h, q->grid_blocks, (uint64_t)q->n)), dim3(kBlock), 0, h->stream, q->io, (long long)q->n,
                       obs, act_a, act_b, reward, terminated, next_obs);
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

// members per pass through the host staging block of read / load (32 MB of interleaved rows at most, one member at least)
static size_t pop_chunk(size_t nS) { return std::max<size_t>(1, (size_t(32) << 20) / (nS * 80)); }

extern "C" int soccer_q_population_read(soccer_handle* h, soccer_q_population* q, int64_t first, int64_t count, double* Q_a, double* Q_b,
                                        double* alpha, uint64_t* steps) {
    if (int rc = pop_check(h, q, "soccer_q_population_read")) return rc;
    if (int rc = pop_range_check(h, q, "soccer_q_population_read", first, count)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const PopIO& io = q->io;
    const size_t nS = (size_t)io.nS, per = nS * 10;
    if (alpha && count) HIP_TRY(h, hipMemcpyAsync(alpha, io.alpha + first, (size_t)count * 8, hipMemcpyDeviceToHost, h->stream));
    if (steps) HIP_TRY(h, hipMemcpyAsync(steps, io.steps, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (Q_a || Q_b) {
        // the device keeps A's and B's row of a state side by side: through a host block, apart again here
        const size_t chunk = pop_chunk(nS);
        std::vector<double> stage;
        for (size_t m0 = 0; m0 < (size_t)count; m0 += chunk) {
            const size_t m = std::min(chunk, (size_t)count - m0);
            stage.resize(m * per);
            HIP_TRY(h, hipMemcpy(stage.data(), io.Q + ((size_t)first + m0) * per, m * per * 8, hipMemcpyDeviceToHost));
            for (size_t r = 0; r < m * nS; ++r)
                for (int k = 0; k < 5; ++k) {
                    if (Q_a) Q_a[(m0 * nS + r) * 5 + k] = stage[r * 10 + k];
                    if (Q_b) Q_b[(m0 * nS + r) * 5 + k] = stage[r * 10 + 5 + k];
                }
        }
    }
    return SOCCER_OK;
}

extern "C" int soccer_q_population_load(soccer_handle* h, soccer_q_population* q, int64_t first, int64_t count, const double* Q_a,
                                        const double* Q_b, const double* alpha, const uint64_t* steps) {
    if (int rc = pop_check(h, q, "soccer_q_population_load")) return rc;
    if (int rc = pop_range_check(h, q, "soccer_q_population_load", first, count)) return rc;
    const PopIO& io = q->io;
    const size_t nS = (size_t)io.nS, per = nS * 10;
    const double* Q[2] = {Q_a, Q_b};
    // everything is checked before anything is written
    for (int p = 0; p < 2; ++p) {
        if (!Q[p]) continue;
        for (size_t i = 0; i < (size_t)count * nS * 5; ++i) {
            if (i / 5 % nS == 0) continue;                  // row 0 is not read
            if (!(Q[p][i] >= -1.0 && Q[p][i] <= 1.0))
                return fail(h, SOCCER_E_INVALID, "soccer_q_population_load: Q_%c[%zu][%zu][%zu] is outside [-1, 1]", p ? 'b' : 'a',
                            i / 5 / nS, i / 5 % nS, i % 5);
        }
    }
    if (alpha)
        for (size_t i = 0; i < (size_t)count; ++i)
            if (!(alpha[i] >= 0.0 && alpha[i] <= 1.0)) return fail(h, SOCCER_E_INVALID, "soccer_q_population_load: alpha[%zu] must be in [0, 1]", i);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (Q_a || Q_b) {
        const size_t chunk = pop_chunk(nS);
        std::vector<double> stage;
        for (size_t m0 = 0; m0 < (size_t)count; m0 += chunk) {
            const size_t m = std::min(chunk, (size_t)count - m0);
            double* const dev = io.Q + ((size_t)first + m0) * per;
            stage.resize(m * per);
            if (!Q_a || !Q_b) HIP_TRY(h, hipMemcpy(stage.data(), dev, m * per * 8, hipMemcpyDeviceToHost));   // the other player's rows stay
            for (size_t r = 0; r < m * nS; ++r)
                for (int p = 0; p < 2; ++p)
                    if (Q[p])
                        for (int k = 0; k < 5; ++k) stage[r * 10 + 5 * p + k] = r % nS == 0 ? 0.0 : Q[p][(m0 * nS + r) * 5 + k];
            HIP_TRY(h, hipMemcpy(dev, stage.data(), m * per * 8, hipMemcpyHostToDevice));
        }
    }
    if (alpha && count) HIP_TRY(h, hipMemcpy(io.alpha + first, alpha, (size_t)count * 8, hipMemcpyHostToDevice));
    if (steps) HIP_TRY(h, hipMemcpy(io.steps, steps, 8, hipMemcpyHostToDevice));
    return SOCCER_OK;
}

// =================================================================================================
// populations of policy hill-climbers, a learner per lane: soccer_wolf_population_*
// =================================================================================================
static_assert(kPhcLearn == SOCCER_PHC_LEARN && kPhcUniform == SOCCER_PHC_UNIFORM && kPhcFixed == SOCCER_PHC_FIXED, "the kernels' names of the modes");

static int wpop_check(soccer_handle* h, soccer_wolf_population* q, const char* what) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "%s during graph capture", what);
    if (!q || std::find(h->wolf_populations.begin(), h->wolf_populations.end(), q) == h->wolf_populations.end())
        return fail(h, SOCCER_E_INVALID, "%s: not a population of this handle", what);
    return SOCCER_OK;
}

static int wpop_range_check(soccer_handle* h, const soccer_wolf_population* q, const char* what, int64_t first, int64_t count) {
    if (first < 0 || count < 0 || (uint64_t)first > q->n || (uint64_t)count > q->n - (uint64_t)first)
        return fail(h, SOCCER_E_INVALID, "%s: members %lld .. %lld + %lld are outside the population of %llu", what, (long long)first,
                    (long long)first, (long long)count, q->n);
    return SOCCER_OK;
}

// launch == false (soccer_wolf_population_create): the LDS limit of this handle's run kernel, as launch_act
template <bool SLIP, bool LUT_LDS>
static hipError_t launch_wpop_run(soccer_handle* h, const KernelParams& P, const PhcPopIO& io, bool launch, int grid_blocks) {
    if (!launch)
        return h->smem_bytes > 48 * 1024 ? hipFuncSetAttribute(reinterpret_cast<const void*>(&phc_pop_run_kernel<SLIP, LUT_LDS>),
                                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->smem_bytes) : hipSuccess;
    hipLaunchKernelGGL((phc_pop_run_kernel<SLIP, LUT_LDS>), dim3(pop_grid(h, grid_blocks, P.n)), dim3(kBlock), h->smem_bytes, h->stream, P, io);
    return hipSuccess;
}

static hipError_t wpop_run(soccer_handle* h, const KernelParams& P, const PhcPopIO& io, bool launch, int grid_blocks = 0) {
    return h->slip ? (h->lut_lds ? launch_wpop_run<true, true>(h, P, io, launch, grid_blocks) : launch_wpop_run<true, false>(h, P, io, launch, grid_blocks))
                   : (h->lut_lds ? launch_wpop_run<false, true>(h, P, io, launch, grid_blocks) : launch_wpop_run<false, false>(h, P, io, launch, grid_blocks));
}

// rows first_row.. of `members` policies [nS][5] each, held to what fixed_thresholds holds a fixed policy to
static int wpop_rows_check(soccer_handle* h, const char* what, const char* name, const double* policy, size_t members, int nS, int first_row) {
    for (size_t m = 0; m < members; ++m)
        for (int s = first_row; s < nS; ++s) {
            const double* p = policy + (m * (size_t)nS + (size_t)s) * 5;
            double sum = 0.0;
            for (int k = 0; k < 5; ++k) {
                if (!(p[k] >= 0.0)) return fail(h, SOCCER_E_INVALID, "%s: %s[%zu][%d][%d] is negative or not a number", what, name, m, s, k);
                sum = sum + p[k];
            }
            if (!(std::fabs(sum - 1.0) <= 1e-8 + 1e-5)) return fail(h, SOCCER_E_INVALID, "%s: %s[%zu][%d] does not sum to 1", what, name, m, s);
        }
    return SOCCER_OK;
}

// members per pass through the host staging block of read / load / creation (32 MB at most, one member at least)
static size_t wpop_chunk(size_t nS) { return std::max<size_t>(1, (size_t(32) << 20) / (nS * kPhcRow * 8)); }

static void launch_adopt(soccer_handle* h, double* dst, int dst_slot, const double* src, size_t src_member, size_t src_row, size_t first,
                         size_t count, int nS) {
    if (count)
        hipLaunchKernelGGL(phc_pop_adopt_kernel, dim3(grid_for(h, (uint64_t)count * (uint64_t)nS)), dim3(kBlock), 0, h->stream, dst, dst_slot, src,
                           (unsigned long long)src_member, (unsigned long long)src_row, (unsigned long long)first, (unsigned long long)count,
                           (int32_t)nS);
}

extern "C" int soccer_wolf_population_create(soccer_handle* h, const soccer_wolf_population_config* cfg, soccer_wolf_population** out) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_wolf_population_create during graph capture");
    if (!cfg || !out) return fail(h, SOCCER_E_INVALID, "soccer_wolf_population_create: cfg/out is NULL");
    *out = nullptr;
    if (h->P.policy_a != nullptr || h->P.policy_b != nullptr)
        return fail(h, SOCCER_E_INVALID, "soccer_wolf_population_create needs a two-player handle: neither side may have a fixed policy (soccer_set_policy)");
    if (!(h->cfg.flags & SOCCER_F_AUTORESET))
        return fail(h, SOCCER_E_INVALID, "soccer_wolf_population_create needs a handle created with SOCCER_F_AUTORESET");
    const size_t n = (size_t)h->cfg.n_lanes;
    const auto unit = [](double x) { return x >= 0.0 && x <= 1.0; };
    const auto factor = [](double x) { return x > 0.0 && x <= 1.0; };
    std::vector<double> par[7];         // alpha, decay, explor, discount_factor, delta_win, delta_lose, delta_decay
    if (int rc = pop_param(h, "discount_factor", "[0, 1)", cfg->discount_factor_per_member, cfg->discount_factor, n,
                           [](double x) { return x >= 0.0 && x < 1.0; }, par[3])) return rc;
    if (int rc = pop_param(h, "alpha", "[0, 1]", cfg->alpha_per_member, cfg->alpha, n, unit, par[0])) return rc;
    if (int rc = pop_param(h, "decay", "(0, 1]", cfg->decay_per_member, cfg->decay, n, factor, par[1])) return rc;
    if (int rc = pop_param(h, "explor", "[0, 1]", cfg->explor_per_member, cfg->explor, n, unit, par[2])) return rc;
    if (!(cfg->q_init >= -1.0 && cfg->q_init <= 1.0)) return fail(h, SOCCER_E_INVALID, "q_init must be in [-1, 1]");
    if (int rc = pop_param(h, "delta_win", "[0, 1]", cfg->delta_win_per_member, cfg->delta_win, n, unit, par[4])) return rc;
    if (int rc = pop_param(h, "delta_lose", "[0, 1]", cfg->delta_lose_per_member, cfg->delta_lose, n, unit, par[5])) return rc;
    if (int rc = pop_param(h, "delta_decay", "(0, 1]", cfg->delta_decay_per_member, cfg->delta_decay, n, factor, par[6])) return rc;
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
        // (row 0 included, as fixed_thresholds checks it; a shared policy is member 0 of one)
        if (shared[p]) if (int rc = wpop_rows_check(h, "soccer_wolf_population_create", names[p][0], shared[p], 1, nS, 0)) return rc;
        if (each[p]) if (int rc = wpop_rows_check(h, "soccer_wolf_population_create", names[p][1], each[p], n, nS, 0)) return rc;
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, wpop_run(h, h->P, PhcPopIO{}, false));
    std::unique_ptr<soccer_wolf_population> owner(new soccer_wolf_population());
    soccer_wolf_population* q = owner.get();
    q->h = h; q->n = n;
    if (const char* e = std::getenv("SOCCER_POP_LAUNCH_STEPS")) {      // (tests: a launch boundary within a short run)
        const long v = std::atol(e);
        if (v >= 1 && v <= 4096) q->launch_steps = (int)v;
    }
    q->grid_blocks = pop_grid_blocks_env(h);
    PhcPopIO& io = q->io;
    double* dpar[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t per = (size_t)nS * kPhcRow, chunk = std::min(wpop_chunk((size_t)nS), n);
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
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // the vectors are pageable host memory of this call
    h->wolf_populations.push_back(q);
    *out = owner.release();
    return SOCCER_OK;
}

extern "C" int soccer_wolf_population_destroy(soccer_handle* h, soccer_wolf_population* q) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (!q) return SOCCER_OK;
    if (int rc = wpop_check(h, q, "soccer_wolf_population_destroy")) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // nothing is freed under a kernel that reads it
    h->wolf_populations.erase(std::find(h->wolf_populations.begin(), h->wolf_populations.end(), q));
    delete q;
    return SOCCER_OK;
}

extern "C" int soccer_wolf_population_run(soccer_handle* h, soccer_wolf_population* q, int32_t n_steps) {
    if (int rc = wpop_check(h, q, "soccer_wolf_population_run")) return rc;
    if (n_steps < 0) return fail(h, SOCCER_E_INVALID, "soccer_wolf_population_run: n_steps must be >= 0");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    // (as soccer_q_population_run: contiguous ticks, a member's whole state in memory between launches)
    for (int32_t t0 = 0; t0 < n_steps; t0 += q->launch_steps) {
        KernelParams P = h->P;
        PhcPopIO io = q->io;
        io.n_steps = n_steps - t0 < q->launch_steps ? n_steps - t0 : q->launch_steps;
        bind_tick(h, P, (uint64_t)io.n_steps);
        HIP_TRY(h, wpop_run(h, P, io, true, q->grid_blocks));
    }
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

extern "C" int soccer_wolf_population_update(soccer_handle* h, soccer_wolf_population* q, const uint16_t* obs, const int8_t* act_a,
                                             const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs) {
    if (int rc = wpop_check(h, q, "soccer_wolf_population_update")) return rc;
    if (!obs || !act_a || !act_b || !reward || !terminated || !next_obs)
        return fail(h, SOCCER_E_INVALID, "soccer_wolf_population_update: all six transition arrays are required");
    if (!aligned(obs, 2) || !aligned(next_obs, 2)) return fail(h, SOCCER_E_INVALID, "soccer_wolf_population_update: obs / next_obs must be 2-byte aligned");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipLaunchKernelGGL(phc_pop_update_kernel, dim3(pop_grid(h, q->grid_blocks, (uint64_t)q->n)), dim3(kBlock), 0, h->stream, q->io, (long long)q->n,
                       obs, act_a, act_b, reward, terminated, next_obs);
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

// the slot of a state's row at which each of the six float64 arrays of soccer_wolf_population_state begins
static const int kWpopSlots[6] = {0, 5, kPhcPi, kPhcPi + kPhcPlayer, kPhcAvg, kPhcAvg + kPhcPlayer};

extern "C" int soccer_wolf_population_read(soccer_handle* h, soccer_wolf_population* q, int64_t first, int64_t count,
                                           const soccer_wolf_population_state* out) {
    if (int rc = wpop_check(h, q, "soccer_wolf_population_read")) return rc;
    if (int rc = wpop_range_check(h, q, "soccer_wolf_population_read", first, count)) return rc;
    if (!out) return fail(h, SOCCER_E_INVALID, "soccer_wolf_population_read: out is NULL");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const PhcPopIO& io = q->io;
    const size_t nS = (size_t)io.nS, per = nS * kPhcRow;
    if (out->alpha && count) HIP_TRY(h, hipMemcpyAsync(out->alpha, io.alpha + first, (size_t)count * 8, hipMemcpyDeviceToHost, h->stream));
    if (out->dscale && count) HIP_TRY(h, hipMemcpyAsync(out->dscale, io.dscale + first, (size_t)count * 8, hipMemcpyDeviceToHost, h->stream));
    if (out->steps) HIP_TRY(h, hipMemcpyAsync(out->steps, io.steps, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    double* const rows[6] = {out->Q_a, out->Q_b, out->pi_a, out->pi_b, out->avg_a, out->avg_b};
    bool any = out->updates != nullptr;
    for (int i = 0; i < 6; ++i) any |= rows[i] != nullptr;
    if (any) {
        // the device keeps a state's values side by side: through a host block, apart again here
        const size_t chunk = wpop_chunk(nS);
        std::vector<double> stage;
        for (size_t m0 = 0; m0 < (size_t)count; m0 += chunk) {
            const size_t m = std::min(chunk, (size_t)count - m0);
            stage.resize(m * per);
            HIP_TRY(h, hipMemcpy(stage.data(), io.tab + ((size_t)first + m0) * per, m * per * 8, hipMemcpyDeviceToHost));
            for (size_t r = 0; r < m * nS; ++r) {
                const double* const from = stage.data() + r * kPhcRow;
                for (int i = 0; i < 6; ++i)
                    if (rows[i])
                        for (int k = 0; k < 5; ++k) rows[i][(m0 * nS + r) * 5 + k] = from[kWpopSlots[i] + k];
                if (out->updates) std::memcpy(&out->updates[m0 * nS + r], from + kPhcUpdates, 8);
            }
        }
    }
    return SOCCER_OK;
}

extern "C" int soccer_wolf_population_load(soccer_handle* h, soccer_wolf_population* q, int64_t first, int64_t count,
                                           const soccer_wolf_population_state* in) {
    if (int rc = wpop_check(h, q, "soccer_wolf_population_load")) return rc;
    if (int rc = wpop_range_check(h, q, "soccer_wolf_population_load", first, count)) return rc;
    if (!in) return fail(h, SOCCER_E_INVALID, "soccer_wolf_population_load: in is NULL");
    const PhcPopIO& io = q->io;
    const size_t nS = (size_t)io.nS, per = nS * kPhcRow;
    // a UNIFORM player keeps its constant rows
    const bool has[2] = {io.mode[0] != kPhcUniform, io.mode[1] != kPhcUniform};
    const double* rows[6] = {in->Q_a, in->Q_b, has[0] ? in->pi_a : nullptr, has[1] ? in->pi_b : nullptr,
                             has[0] ? in->avg_a : nullptr, has[1] ? in->avg_b : nullptr};
    static const char* const names[6] = {"Q_a", "Q_b", "pi_a", "pi_b", "avg_a", "avg_b"};
    // everything is checked before anything is written
    for (int p = 0; p < 2; ++p) {
        if (!rows[p]) continue;
        for (size_t i = 0; i < (size_t)count * nS * 5; ++i) {
            if (i / 5 % nS == 0) continue;                  // row 0 is not read
            if (!(rows[p][i] >= -1.0 && rows[p][i] <= 1.0))
                return fail(h, SOCCER_E_INVALID, "soccer_wolf_population_load: %s[%zu][%zu][%zu] is outside [-1, 1]", names[p],
                            i / 5 / nS, i / 5 % nS, i % 5);
        }
    }
    for (int i = 2; i < 6; ++i)
        if (rows[i]) if (int rc = wpop_rows_check(h, "soccer_wolf_population_load", names[i], rows[i], (size_t)count, io.nS, 1)) return rc;
    const double* const scal[2] = {in->alpha, in->dscale};
    for (int j = 0; j < 2; ++j)
        if (scal[j])
            for (size_t i = 0; i < (size_t)count; ++i)
                if (!(scal[j][i] >= 0.0 && scal[j][i] <= 1.0))
                    return fail(h, SOCCER_E_INVALID, "soccer_wolf_population_load: %s[%zu] must be in [0, 1]", j ? "dscale" : "alpha", i);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    bool any = in->updates != nullptr;
    for (int i = 0; i < 6; ++i) any |= rows[i] != nullptr;
    if (any) {
        const size_t chunk = wpop_chunk(nS);
        std::vector<double> stage;
        for (size_t m0 = 0; m0 < (size_t)count; m0 += chunk) {
            const size_t m = std::min(chunk, (size_t)count - m0);
            double* const dev = io.tab + ((size_t)first + m0) * per;
            stage.resize(m * per);
            HIP_TRY(h, hipMemcpy(stage.data(), dev, m * per * 8, hipMemcpyDeviceToHost));          // what is not given stays
            for (size_t r = 0; r < m * nS; ++r) {
                double* const to = stage.data() + r * kPhcRow;
                const bool row0 = r % nS == 0;
                for (int i = 0; i < 6; ++i) {
                    if (!rows[i]) continue;
                    if (row0 && i >= 2) continue;           // row 0 of pi and avg stays what creation gave it
                    for (int k = 0; k < 5; ++k) to[kWpopSlots[i] + k] = row0 ? 0.0 : rows[i][(m0 * nS + r) * 5 + k];
                }
                if (in->updates) std::memcpy(to + kPhcUpdates, &in->updates[m0 * nS + r], 8);
            }
            HIP_TRY(h, hipMemcpy(dev, stage.data(), m * per * 8, hipMemcpyHostToDevice));
        }
    }
    if (in->alpha && count) HIP_TRY(h, hipMemcpy(io.alpha + first, in->alpha, (size_t)count * 8, hipMemcpyHostToDevice));
    if (in->dscale && count) HIP_TRY(h, hipMemcpy(io.dscale + first, in->dscale, (size_t)count * 8, hipMemcpyHostToDevice));
    if (in->steps) HIP_TRY(h, hipMemcpy(io.steps, in->steps, 8, hipMemcpyHostToDevice));
    return SOCCER_OK;
}

extern "C" int soccer_wolf_population_adopt(soccer_handle* h, soccer_wolf_population* dst, int32_t dst_player, soccer_wolf_population* src,
                                            int32_t src_player, int32_t which) {
    if (int rc = wpop_check(h, dst, "soccer_wolf_population_adopt (dst)")) return rc;
    if (int rc = wpop_check(h, src, "soccer_wolf_population_adopt (src)")) return rc;
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

// =================================================================================================
// populations of minimax-Q learners, a learner per lane: soccer_minimax_q_population_*
// =================================================================================================
static_assert(kMqUniform == SOCCER_MQ_UNIFORM && kMqSelf == SOCCER_MQ_SELF && kMqFixed == SOCCER_MQ_FIXED, "the kernels' names of the modes");

static int mqpop_check(soccer_handle* h, soccer_minimax_q_population* q, const char* what) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "%s during graph capture", what);
    if (!q || std::find(h->mq_populations.begin(), h->mq_populations.end(), q) == h->mq_populations.end())
        return fail(h, SOCCER_E_INVALID, "%s: not a population of this handle", what);
    return SOCCER_OK;
}

static int mqpop_range_check(soccer_handle* h, const soccer_minimax_q_population* q, const char* what, int64_t first, int64_t count) {
    if (first < 0 || count < 0 || (uint64_t)first > q->n || (uint64_t)count > q->n - (uint64_t)first)
        return fail(h, SOCCER_E_INVALID, "%s: members %lld .. %lld + %lld are outside the population of %llu", what, (long long)first,
                    (long long)first, (long long)count, q->n);
    return SOCCER_OK;
}

// workgroups of one wave for `items` members (or states): never more than the population's histogram slots allow
static unsigned mqpop_grid(const soccer_minimax_q_population* q, uint64_t items) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(items, q->waves));
}

// members per pass through the host staging block of read / load (32 MB at most, one member at least)
static size_t mqpop_chunk(size_t nS) { return std::max<size_t>(1, (size_t(32) << 20) / (nS * kMqRow * 8)); }

extern "C" int soccer_minimax_q_population_create(soccer_handle* h, const soccer_minimax_q_population_config* cfg,
                                                  soccer_minimax_q_population** out) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_minimax_q_population_create during graph capture");
    if (!cfg || !out) return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_population_create: cfg/out is NULL");
    *out = nullptr;
    if (h->P.policy_a != nullptr || h->P.policy_b != nullptr)
        return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_population_create needs a two-player handle: neither side may have a fixed policy (soccer_set_policy)");
    if (!(h->cfg.flags & SOCCER_F_AUTORESET))
        return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_population_create needs a handle created with SOCCER_F_AUTORESET");
    const size_t n = (size_t)h->cfg.n_lanes;
    std::vector<double> par[4];         // alpha, decay, explor, discount_factor
    if (int rc = pop_param(h, "discount_factor", "[0, 1)", cfg->discount_factor_per_member, cfg->discount_factor, n,
                           [](double x) { return x >= 0.0 && x < 1.0; }, par[3])) return rc;
    if (int rc = pop_param(h, "alpha", "[0, 1]", cfg->alpha_per_member, cfg->alpha, n, [](double x) { return x >= 0.0 && x <= 1.0; }, par[0])) return rc;
    if (int rc = pop_param(h, "decay", "(0, 1]", cfg->decay_per_member, cfg->decay, n, [](double x) { return x > 0.0 && x <= 1.0; }, par[1])) return rc;
    if (int rc = pop_param(h, "explor", "[0, 1]", cfg->explor_per_member, cfg->explor, n, [](double x) { return x >= 0.0 && x <= 1.0; }, par[2])) return rc;
    if (!(cfg->q_init >= -1.0 && cfg->q_init <= 1.0)) return fail(h, SOCCER_E_INVALID, "q_init must be in [-1, 1]");
    if (cfg->opponent != SOCCER_MQ_UNIFORM && cfg->opponent != SOCCER_MQ_SELF && cfg->opponent != SOCCER_MQ_FIXED)
        return fail(h, SOCCER_E_INVALID, "opponent must be SOCCER_MQ_UNIFORM, SOCCER_MQ_SELF or SOCCER_MQ_FIXED");
    const double* const shared = cfg->opponent_policy;
    const double* const each = cfg->opponent_policy_per_member;
    if ((cfg->opponent == SOCCER_MQ_FIXED) != ((shared != nullptr) != (each != nullptr)) || (shared && each))
        return fail(h, SOCCER_E_INVALID, "exactly one of opponent_policy and opponent_policy_per_member goes with opponent == SOCCER_MQ_FIXED, and neither with another mode");
    const int nS = h->rules.nS;
    // (row 0 included, as fixed_thresholds checks it; a shared policy is member 0 of one)
    if (shared) if (int rc = wpop_rows_check(h, "soccer_minimax_q_population_create", "opponent_policy", shared, 1, nS, 0)) return rc;
    if (each) if (int rc = wpop_rows_check(h, "soccer_minimax_q_population_create", "opponent_policy_per_member", each, n, nS, 0)) return rc;
    std::vector<uint16_t> fixed, one;
    const size_t fixed_members = shared ? 1 : (each ? n : 0);
    for (size_t m = 0; m < fixed_members; ++m) {
        if (int rc = fixed_thresholds(h, "opponent_policy", (shared ? shared : each) + m * (size_t)nS * 5, nS, one)) return rc;
        fixed.insert(fixed.end(), one.begin(), one.end());
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    std::unique_ptr<soccer_minimax_q_population> owner(new soccer_minimax_q_population());
    soccer_minimax_q_population* q = owner.get();
    q->h = h; q->n = n;
    if (const char* e = std::getenv("SOCCER_POP_LAUNCH_STEPS")) {      // (tests: a launch boundary within a short run)
        const long v = std::atol(e);
        if (v >= 1 && v <= 4096) q->launch_steps = (int)v;
    }
    // a workgroup is one wave and owns one histogram slot: as many as the capped grids of the other kernels have waves
    q->waves = (unsigned)std::min<uint64_t>((uint64_t)h->grid_cap * (kBlock / 64), h->hist_slots);
    if (const char* e = std::getenv("SOCCER_MQ_POP_WAVES")) {          // (tests: a wave that serves several members in turn)
        const long v = std::atol(e);
        if (v >= 1 && (unsigned long)v <= q->waves) q->waves = (unsigned)v;
    }
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
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // the vectors are pageable host memory of this call
    h->mq_populations.push_back(q);
    *out = owner.release();
    return SOCCER_OK;
}

extern "C" int soccer_minimax_q_population_destroy(soccer_handle* h, soccer_minimax_q_population* q) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (!q) return SOCCER_OK;
    if (int rc = mqpop_check(h, q, "soccer_minimax_q_population_destroy")) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // nothing is freed under a kernel that reads it
    h->mq_populations.erase(std::find(h->mq_populations.begin(), h->mq_populations.end(), q));
    delete q;
    return SOCCER_OK;
}

extern "C" int soccer_minimax_q_population_run(soccer_handle* h, soccer_minimax_q_population* q, int32_t n_steps) {
    if (int rc = mqpop_check(h, q, "soccer_minimax_q_population_run")) return rc;
    if (n_steps < 0) return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_population_run: n_steps must be >= 0");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    // (as soccer_q_population_run: contiguous ticks, a member's whole state in memory between launches)
    for (int32_t t0 = 0; t0 < n_steps; t0 += q->launch_steps) {
        KernelParams P = h->P;
        MqPopIO io = q->io;
        io.n_steps = n_steps - t0 < q->launch_steps ? n_steps - t0 : q->launch_steps;
        bind_tick(h, P, (uint64_t)io.n_steps);
        const dim3 grid(mqpop_grid(q, P.n));
        if (h->slip) hipLaunchKernelGGL(mq_pop_run_kernel<true>, grid, dim3(kMqBlock), 0, h->stream, P, io);
        else hipLaunchKernelGGL(mq_pop_run_kernel<false>, grid, dim3(kMqBlock), 0, h->stream, P, io);
    }
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

extern "C" int soccer_minimax_q_population_update(soccer_handle* h, soccer_minimax_q_population* q, const uint16_t* obs, const int8_t* act_a,
                                                  const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs) {
    if (int rc = mqpop_check(h, q, "soccer_minimax_q_population_update")) return rc;
    if (!obs || !act_a || !act_b || !reward || !terminated || !next_obs)
        return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_population_update: all six transition arrays are required");
    if (!aligned(obs, 2) || !aligned(next_obs, 2)) return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_population_update: obs / next_obs must be 2-byte aligned");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipLaunchKernelGGL(mq_pop_update_kernel, dim3(mqpop_grid(q, q->n)), dim3(kMqBlock), 0, h->stream, q->io, (long long)q->n,
                       obs, act_a, act_b, reward, terminated, next_obs);
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

// the slot of a state's row at which each of the four arrays begins, and how many values it has there
static const int kMqSlots[4] = {0, kMqV, kMqPiA, kMqPiB};
static const int kMqWidth[4] = {25, 1, 5, 5};

extern "C" int soccer_minimax_q_population_read(soccer_handle* h, soccer_minimax_q_population* q, int64_t first, int64_t count, double* Q,
                                                double* V, double* pi_a, double* pi_b, double* alpha, uint64_t* steps) {
    if (int rc = mqpop_check(h, q, "soccer_minimax_q_population_read")) return rc;
    if (int rc = mqpop_range_check(h, q, "soccer_minimax_q_population_read", first, count)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const MqPopIO& io = q->io;
    const size_t nS = (size_t)io.nS, per = nS * kMqRow;
    if (alpha && count) HIP_TRY(h, hipMemcpyAsync(alpha, io.alpha + first, (size_t)count * 8, hipMemcpyDeviceToHost, h->stream));
    if (steps) HIP_TRY(h, hipMemcpyAsync(steps, io.steps, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    double* const rows[4] = {Q, V, pi_a, pi_b};
    if (Q || V || pi_a || pi_b) {
        // the device keeps a state's values side by side: through a host block, apart again here
        const size_t chunk = mqpop_chunk(nS);
        std::vector<double> stage;
        for (size_t m0 = 0; m0 < (size_t)count; m0 += chunk) {
            const size_t m = std::min(chunk, (size_t)count - m0);
            stage.resize(m * per);
            HIP_TRY(h, hipMemcpy(stage.data(), io.tab + ((size_t)first + m0) * per, m * per * 8, hipMemcpyDeviceToHost));
            for (size_t r = 0; r < m * nS; ++r) {
                const double* const from = stage.data() + r * kMqRow;
                for (int i = 0; i < 4; ++i)
                    if (rows[i])
                        for (int k = 0; k < kMqWidth[i]; ++k) rows[i][(m0 * nS + r) * kMqWidth[i] + k] = from[kMqSlots[i] + k];
            }
        }
    }
    return SOCCER_OK;
}

extern "C" int soccer_minimax_q_population_load(soccer_handle* h, soccer_minimax_q_population* q, int64_t first, int64_t count, const double* Q,
                                                const double* V, const double* pi_a, const double* pi_b, const double* alpha,
                                                const uint64_t* steps) {
    if (int rc = mqpop_check(h, q, "soccer_minimax_q_population_load")) return rc;
    if (int rc = mqpop_range_check(h, q, "soccer_minimax_q_population_load", first, count)) return rc;
    const MqPopIO& io = q->io;
    const size_t nS = (size_t)io.nS, per = nS * kMqRow;
    const double* const rows[4] = {Q, V, pi_a, pi_b};
    // everything is checked before anything is written
    if (Q)
        for (size_t i = 0; i < (size_t)count * nS * 25; ++i) {
            if (i / 25 % nS == 0) continue;                 // row 0 is not read
            if (!(Q[i] >= -1.0 && Q[i] <= 1.0))
                return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_population_load: Q[%zu][%zu][%zu][%zu] is outside [-1, 1]", i / 25 / nS,
                            i / 25 % nS, i % 25 / 5, i % 5);
        }
    if (V)
        for (size_t i = 0; i < (size_t)count * nS; ++i) {
            if (i % nS == 0) continue;
            if (!(V[i] >= -1.0 && V[i] <= 1.0))
                return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_population_load: V[%zu][%zu] is outside [-1, 1]", i / nS, i % nS);
        }
    if (pi_a) if (int rc = wpop_rows_check(h, "soccer_minimax_q_population_load", "pi_a", pi_a, (size_t)count, io.nS, 1)) return rc;
    if (pi_b) if (int rc = wpop_rows_check(h, "soccer_minimax_q_population_load", "pi_b", pi_b, (size_t)count, io.nS, 1)) return rc;
    if (alpha)
        for (size_t i = 0; i < (size_t)count; ++i)
            if (!(alpha[i] >= 0.0 && alpha[i] <= 1.0)) return fail(h, SOCCER_E_INVALID, "soccer_minimax_q_population_load: alpha[%zu] must be in [0, 1]", i);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (Q || V || pi_a || pi_b) {
        const size_t chunk = mqpop_chunk(nS);
        std::vector<double> stage;
        for (size_t m0 = 0; m0 < (size_t)count; m0 += chunk) {
            const size_t m = std::min(chunk, (size_t)count - m0);
            double* const dev = io.tab + ((size_t)first + m0) * per;
            stage.resize(m * per);
            HIP_TRY(h, hipMemcpy(stage.data(), dev, m * per * 8, hipMemcpyDeviceToHost));          // what is not given stays
            for (size_t r = 0; r < m * nS; ++r) {
                double* const to = stage.data() + r * kMqRow;
                const bool row0 = r % nS == 0;
                for (int i = 0; i < 4; ++i) {
                    if (!rows[i]) continue;
                    if (row0 && i >= 2) continue;           // row 0 of the strategies stays what creation gave it
                    for (int k = 0; k < kMqWidth[i]; ++k) to[kMqSlots[i] + k] = row0 ? 0.0 : rows[i][(m0 * nS + r) * kMqWidth[i] + k];
                }
            }
            HIP_TRY(h, hipMemcpy(dev, stage.data(), m * per * 8, hipMemcpyHostToDevice));
        }
    }
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
