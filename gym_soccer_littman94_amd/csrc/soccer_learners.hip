// soccer_learners.hip — the minimax-Q learner: soccer_minimax_q_* (see soccer_handle.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
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

void learners_release(soccer_handle* h) {
    for (soccer_minimax_q* q : h->learners) delete q;
    h->learners.clear();
}

// what every entry point checks first
static int learner_check(soccer_handle* h, soccer_minimax_q* q, const char* what) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "%s during graph capture", what);
    if (!owns(h, q)) return fail(h, SOCCER_E_INVALID, "%s: not a learner of this handle", what);
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
    // a fixed opponent's threshold rows, once: SoccerBatch.mixed_policy_thresholds
    std::vector<uint16_t> fixed;
    if (cfg->opponent == SOCCER_MQ_FIXED) {
        fixed.resize((size_t)nS * 4);
        for (int s = 0; s < nS; ++s) {
            const double* p = cfg->opponent_policy + (size_t)s * 5;
            double c = 0.0, sum = 0.0;
            for (int k = 0; k < 5; ++k) {
                if (!(p[k] >= 0.0)) return fail(h, SOCCER_E_INVALID, "opponent_policy[%d][%d] is negative or not a number", s, k);
                sum = sum + p[k];
            }
            if (!(std::fabs(sum - 1.0) <= 1e-8 + 1e-5)) return fail(h, SOCCER_E_INVALID, "opponent_policy[%d] does not sum to 1", s);
            for (int k = 0; k < 4; ++k) {
                c = c + p[k];
                double f = std::floor(c * 32768.0 + 1e-9);
                f = f < 0.0 ? 0.0 : (f > 32768.0 ? 32768.0 : f);
                fixed[(size_t)s * 4 + k] = (uint16_t)f;
            }
        }
    }
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
