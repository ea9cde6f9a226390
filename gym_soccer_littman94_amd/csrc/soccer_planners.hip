// soccer_planners.hip — the transition table, the single-agent planners, minimax value iteration, best responses to mixed policies, cross-play, match outcomes, state occupancy, policy gradients with gradient play, and the matrix-game solver (see soccer_handle.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstring>
#include <utility>
#include <vector>

#include "soccer_handle.hpp"
#include "soccer_planner_kernels.hpp"

// the reference's P_readable, computed on the device by the rule functions of the step kernels
extern "C" int soccer_enumerate_transitions(soccer_handle* h, int32_t* count, double* prob, int32_t* next_flat,
                                            int8_t* reward, uint8_t* done) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_enumerate_transitions during graph capture");
    if (!count || !prob || !next_flat || !reward || !done) return fail(h, SOCCER_E_INVALID, "all five outputs are required");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t keys = h->rules.lut.size() * 25, ent = keys * kMaxOutcomes;
    EnumIO io{};
    io.n_tuples = static_cast<int32_t>(h->rules.lut.size()); io.H = h->rules.H;
    OwnedBufs tmp("the transition table");                              // freed on every way out
    int rc = tmp.alloc(h, keys, &io.count);
    if (!rc) rc = tmp.alloc(h, ent, &io.prob);
    if (!rc) rc = tmp.alloc(h, ent, &io.next);
    if (!rc) rc = tmp.alloc(h, ent, &io.reward);
    if (!rc) rc = tmp.alloc(h, ent, &io.done);
    if (rc) return rc;
    const unsigned grid = static_cast<unsigned>((keys + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(enumerate_kernel, dim3(grid), dim3(kBlock), 0, h->stream, h->P, io);
    void* dst[5] = {count, prob, next_flat, reward, done};
    const void* src[5] = {io.count, io.prob, io.next, io.reward, io.done};
    const size_t sizes[5] = {keys * sizeof(int32_t), ent * sizeof(double), ent * sizeof(int32_t), ent, ent};
    hipError_t e = hipGetLastError();
    for (int i = 0; i < 5 && e == hipSuccess; ++i) e = hipMemcpyAsync(dst[i], src[i], sizes[i], hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, SOCCER_E_HIP, "transition table export failed: %s", hipGetErrorString(e));
    return SOCCER_OK;
}

// ------------------------------------------------------------------------------------------------
// planners (reference gym_soccer/utils/planners.py).  The (state, learner action) lists are assembled on
// the host from the device-enumerated transition relation exactly as the reference's constructor builds
// P[s][a], Pmat and Rmat (:167-293), cached on the handle until the policy changes, and one
// single-workgroup kernel runs the whole planner.
static int build_plan(soccer_handle* h) {
    if (h->plan_bufs.ready) return SOCCER_OK;
    const bool fixed_a = h->P.policy_a != nullptr, fixed_b = h->P.policy_b != nullptr;
    if (fixed_a == fixed_b)
        return fail(h, SOCCER_E_INVALID, "planners need single-agent mode: exactly one side with a fixed policy (soccer_set_policy)");
    const Rules& R = h->rules;
    const int nS = R.nS;
    if ((size_t)nS * sizeof(double) > 150 * 1024) return fail(h, SOCCER_E_INVALID, "too many states (%d) for the single-workgroup planner", nS);
    const size_t T = R.lut.size(), keys = T * 25, ent = keys * kMaxOutcomes;
    std::vector<int32_t> count(keys), nxt(ent); std::vector<double> prob(ent); std::vector<int8_t> rew(ent); std::vector<uint8_t> done(ent);
    if (int rc = soccer_enumerate_transitions(h, count.data(), prob.data(), nxt.data(), rew.data(), done.data())) return rc;
    std::vector<int8_t> policy(nS);
    HIP_TRY(h, hipMemcpy(policy.data(), fixed_a ? h->P.policy_a : h->P.policy_b, (size_t)nS, hipMemcpyDeviceToHost));
    auto obs_of = [&](size_t f) { return R.kind[f] == 2 ? 0 : (int)R.lut[f]; };
    const bool flip = fixed_a;                                          // learner B sees -r (:243-244)
    // P[s][a]: goal tuples all write index 0 and overwrite each other (identical lists), live tuples own theirs
    std::vector<long> tuple_of(nS, -1);
    for (size_t f = 0; f < T; ++f) if (R.kind[f] != 0) tuple_of[obs_of(f)] = (long)f;
    const PlanEntry pad_entry{0.0, (int32_t)0x80000000, 0.0f};
    auto pad = [&](std::vector<PlanEntry>& v) { while (v.size() % kPlanPad) v.push_back(pad_entry); };
    std::vector<int32_t> off((size_t)nS * 5 + 1, 0); std::vector<PlanEntry> lists;
    for (int s = 0; s < nS; ++s) for (int a = 0; a < 5; ++a) {
        const long f = tuple_of[s];
        if (f < 0) return fail(h, SOCCER_E_INVALID, "internal error: observation index %d has no tuple", s);
        const size_t key = (size_t)f * 25 + (fixed_a ? policy[s] : a) * 5 + (fixed_b ? policy[s] : a);
        for (int k = 0; k < count[key]; ++k) {
            const size_t e = key * kMaxOutcomes + k;
            const double rr = flip ? -1.0 * (double)rew[e] : (double)rew[e];
            lists.push_back(PlanEntry{prob[e], obs_of((size_t)nxt[e]) | (done[e] ? (int32_t)0x80000000 : 0), (float)rr});
        }
        pad(lists);
        off[(size_t)s * 5 + a + 1] = (int32_t)lists.size();
    }
    // Pmat[s][ns][a] += p and Rmat[s][a] (= 0, then += p * r) in the constructor's tuple order (:280-291):
    // index 0 accumulates one unit of probability per goal tuple, its Rmat is the last goal tuple's (0).
    // A row of Pmat is kept as its touched next states only (a few dozen of nS; full rows for every (s, a) would be
    // nS^2 * 40 bytes, 5.5 GB at 11x7); each accumulates its probabilities in tuple and entry order, as a dense row would.
    std::vector<std::vector<std::pair<int32_t, double>>> row((size_t)nS * 5);
    std::vector<double> Rm((size_t)nS * 5, 0.0);
    for (size_t f = 0; f < T; ++f) {
        if (R.kind[f] == 0) continue;
        const int s = obs_of(f);
        for (int a = 0; a < 5; ++a) {
            const size_t key = f * 25 + (fixed_a ? policy[s] : a) * 5 + (fixed_b ? policy[s] : a);
            std::vector<std::pair<int32_t, double>>& r = row[(size_t)s * 5 + a];
            double acc = 0.0;
            for (int k = 0; k < count[key]; ++k) {
                const size_t e = key * kMaxOutcomes + k;
                const double rr = flip ? -1.0 * (double)rew[e] : (double)rew[e];
                const int32_t ns = obs_of((size_t)nxt[e]);
                auto it = std::find_if(r.begin(), r.end(), [ns](const std::pair<int32_t, double>& x) { return x.first == ns; });
                if (it == r.end()) r.emplace_back(ns, 0.0 + prob[e]);
                else it->second += prob[e];
                acc = acc + prob[e] * rr;
            }
            Rm[(size_t)s * 5 + a] = acc;
        }
    }
    // ascending next state, exact zeros dropped: the entries a scan of the dense row would emit
    std::vector<int32_t> m_off((size_t)nS * 5 + 1, 0); std::vector<PlanEntry> m_lists;
    const PlanEntry m_pad{0.0, 0, 0.0f};
    for (size_t q = 0; q < (size_t)nS * 5; ++q) {
        std::sort(row[q].begin(), row[q].end());                        // next states are distinct within a row
        for (const auto& x : row[q]) if (x.second != 0.0) m_lists.push_back(PlanEntry{x.second, x.first, 0.0f});
        while (m_lists.size() % kPlanPad) m_lists.push_back(m_pad);
        m_off[q + 1] = (int32_t)m_lists.size();
        std::vector<std::pair<int32_t, double>>().swap(row[q]);
    }
    PlanIO& io = h->plan;
    io = PlanIO{};
    int rc = h->plan_bufs.upload(h, off, &io.offset);
    if (!rc) rc = h->plan_bufs.upload(h, lists, &io.list);
    if (!rc) rc = h->plan_bufs.upload(h, m_off, &io.m_offset);
    if (!rc) rc = h->plan_bufs.upload(h, m_lists, &io.m_list);
    if (!rc) rc = h->plan_bufs.upload(h, Rm, &io.m_R);
    const std::vector<double> zV(nS, 0.0), zQ((size_t)nS * 5, 0.0); const std::vector<int32_t> zpi(nS, 0), zc(16, 0);
    const double* cV = nullptr; const double* cN = nullptr; const double* cQ = nullptr; const int32_t* cpi = nullptr; const int32_t* cc = nullptr;
    if (!rc) rc = h->plan_bufs.upload(h, zV, &cV);
    if (!rc) rc = h->plan_bufs.upload(h, zV, &cN);
    if (!rc) rc = h->plan_bufs.upload(h, zQ, &cQ);
    if (!rc) rc = h->plan_bufs.upload(h, zpi, &cpi);
    if (!rc) rc = h->plan_bufs.upload(h, zc, &cc);
    if (rc) { h->plan_bufs.clear(); return rc; }
    io.V = const_cast<double*>(cV); io.newV = const_cast<double*>(cN); io.Q = const_cast<double*>(cQ);
    io.pi = const_cast<int32_t*>(cpi); io.counters = const_cast<int32_t*>(cc);
    io.nS = nS;
    const size_t smem = (size_t)nS * sizeof(double);
    if (smem > 48 * 1024)
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&planner_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    h->plan_bufs.ready = true;
    return SOCCER_OK;
}

// runs one planner; inputs pi_in / V_in and every output are HOST pointers (any output may be NULL)
static int run_plan(soccer_handle* h, const char* what, int mode, double theta, double gamma, int32_t max_sweeps, int32_t k,
                    const int32_t* pi_in, const double* V_in, const double* Q_in, double* V, double* Q, int32_t* pi, int32_t* iterations) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "%s during graph capture", what);
    if (max_sweeps < 1) return fail(h, SOCCER_E_INVALID, "max_sweeps must be >= 1");
    if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(h, SOCCER_E_INVALID, "discount_factor must be in [0, 1]");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (int rc = build_plan(h)) return rc;
    PlanIO io = h->plan;
    const int nS = io.nS;
    if (pi_in) {
        for (int s = 0; s < nS; ++s) if (pi_in[s] < 0 || pi_in[s] > 4) return fail(h, SOCCER_E_INVALID, "pi[%d] = %d is not an action", s, pi_in[s]);
        HIP_TRY(h, hipMemcpyAsync(io.pi, pi_in, (size_t)nS * 4, hipMemcpyHostToDevice, h->stream));
    }
    if (V_in) HIP_TRY(h, hipMemcpyAsync(io.V, V_in, (size_t)nS * 8, hipMemcpyHostToDevice, h->stream));
    else if (mode == kPlanEvalDense) HIP_TRY(h, hipMemsetAsync(io.V, 0, (size_t)nS * 8, h->stream));
    if (Q_in) HIP_TRY(h, hipMemcpyAsync(io.Q, Q_in, (size_t)nS * 40, hipMemcpyHostToDevice, h->stream));
    io.mode = mode; io.theta = theta; io.gamma = gamma; io.max_sweeps = max_sweeps; io.k = k;
    io.threshold = (theta * (1 - gamma)) / (2 * gamma);                  // planners.py:75
    hipLaunchKernelGGL(planner_kernel, dim3(1), dim3(1024), (size_t)nS * sizeof(double), h->stream, io);
    HIP_TRY(h, hipGetLastError());
    int32_t counters[4] = {0, 0, 0, 0};
    if (V) HIP_TRY(h, hipMemcpyAsync(V, io.V, (size_t)nS * 8, hipMemcpyDeviceToHost, h->stream));
    if (Q) HIP_TRY(h, hipMemcpyAsync(Q, io.Q, (size_t)nS * 40, hipMemcpyDeviceToHost, h->stream));
    if (pi) HIP_TRY(h, hipMemcpyAsync(pi, io.pi, (size_t)nS * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(counters, io.counters, 12, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (iterations) *iterations = counters[0];
    if (counters[2]) return fail(h, SOCCER_E_STATE, "%s stopped after max_sweeps = %d sweeps without converging", what, max_sweeps);
    return SOCCER_OK;
}

extern "C" int soccer_value_iteration(soccer_handle* h, double theta, double discount_factor, int32_t max_sweeps,
                                      double* V, double* Q, int32_t* pi, int32_t* iterations) {
    return run_plan(h, "soccer_value_iteration", kPlanVI, theta, discount_factor, max_sweeps, 0, nullptr, nullptr, nullptr, V, Q, pi, iterations);
}

extern "C" int soccer_policy_evaluation(soccer_handle* h, const int32_t* pi, double theta, double discount_factor,
                                        int32_t max_sweeps, double* V, int32_t* sweeps) {
    if (h && !pi) return fail(h, SOCCER_E_INVALID, "pi is NULL");
    return run_plan(h, "soccer_policy_evaluation", kPlanEval, theta, discount_factor, max_sweeps, 0, pi, nullptr, nullptr, V, nullptr, nullptr, sweeps);
}

extern "C" int soccer_policy_improvement(soccer_handle* h, const double* V, double discount_factor, double* Q, int32_t* new_pi) {
    if (h && !V) return fail(h, SOCCER_E_INVALID, "V is NULL");
    return run_plan(h, "soccer_policy_improvement", kPlanImprove, 0.0, discount_factor, 1, 0, nullptr, V, nullptr, nullptr, Q, new_pi, nullptr);
}

extern "C" int soccer_policy_iteration(soccer_handle* h, const int32_t* pi0, double theta, double discount_factor,
                                       int32_t max_sweeps, double* V, double* Q, int32_t* pi, int32_t* iterations) {
    if (h && !pi0) return fail(h, SOCCER_E_INVALID, "pi0 (the initial policy) is NULL");
    return run_plan(h, "soccer_policy_iteration", kPlanPI, theta, discount_factor, max_sweeps, 0, pi0, nullptr, nullptr, V, Q, pi, iterations);
}

extern "C" int soccer_modified_policy_iteration(soccer_handle* h, int32_t k, double theta, double discount_factor,
                                                int32_t max_sweeps, double* V, double* Q, int32_t* pi, int32_t* iterations) {
    if (h && k < 1) return fail(h, SOCCER_E_INVALID, "k must be >= 1");
    if (h && !(discount_factor > 0.0)) return fail(h, SOCCER_E_INVALID, "discount_factor must be > 0 for the stopping threshold");
    return run_plan(h, "soccer_modified_policy_iteration", kPlanMPI, theta, discount_factor, max_sweeps, k, nullptr, nullptr, nullptr, V, Q, pi, iterations);
}

extern "C" int soccer_policy_eval_dense(soccer_handle* h, const double* policy, int32_t k, double theta, double discount_factor,
                                        int32_t max_sweeps, const double* init, double* v, int32_t* sweeps) {
    if (h && !policy) return fail(h, SOCCER_E_INVALID, "policy is NULL");
    if (h && k < 1) return fail(h, SOCCER_E_INVALID, "k must be >= 1");
    return run_plan(h, "soccer_policy_eval_dense", kPlanEvalDense, theta, discount_factor, max_sweeps, k, nullptr, init, policy, v, nullptr, nullptr, sweeps);
}

// ------------------------------------------------------------------------------------------------
// minimax value iteration (two-player handles).  The (state, joint action) lists are the ones build_plan would assemble
// for a joint action (P[0] = the last goal tuple's lists, player A's reward), built on the device from enumerate_kernel's
// output without a round trip of the transition relation through the host (at 11x7 that copy and the host loops were 95 %
// of a solve), cached on the handle apart from the single-agent plan; every sweep is one launch of minimax_sweep_kernel
// over the whole GPU.
constexpr int kMinimaxBatch = 16;             // sweeps enqueued between two synchronisations

static int build_minimax(soccer_handle* h) {
    if (h->mm_bufs.ready) return SOCCER_OK;
    const Rules& R = h->rules;
    const int nS = R.nS;
    const size_t T = R.lut.size(), keys = T * 25, ent = keys * kMaxOutcomes, nkeys = (size_t)nS * 25;
    // P[s]: goal tuples all write index 0 and overwrite each other (identical lists), live tuples own theirs
    std::vector<int32_t> tuple_of(nS, -1);
    for (size_t f = 0; f < T; ++f) if (R.kind[f] != 0) tuple_of[R.kind[f] == 2 ? 0 : (int)R.lut[f]] = (int32_t)f;
    for (int s = 0; s < nS; ++s) if (tuple_of[s] < 0) return fail(h, SOCCER_E_INVALID, "internal error: observation index %d has no tuple", s);
    // the transition relation stays on the device: enumerate, measure the lists, place them
    OwnedBufs tmp("the transition table");                              // freed below, or on an earlier way out
    EnumIO io{};
    io.n_tuples = static_cast<int32_t>(T); io.H = R.H;
    int32_t* d_tuple_of = nullptr;
    int rc = tmp.alloc(h, keys, &io.count);
    if (!rc) rc = tmp.alloc(h, ent, &io.prob);
    if (!rc) rc = tmp.alloc(h, ent, &io.next);
    if (!rc) rc = tmp.alloc(h, ent, &io.reward);
    if (!rc) rc = tmp.alloc(h, ent, &io.done);
    if (!rc) rc = tmp.alloc(h, (size_t)nS, &d_tuple_of);
    int32_t* d_off = nullptr; PlanEntry* d_list = nullptr;
    std::vector<int32_t> off(nkeys + 1, 0);
    MinimaxListIO L{};
    hipError_t e = hipSuccess;
    if (rc == SOCCER_OK) rc = h->mm_bufs.alloc(h, off.size(), &d_off);
    if (rc == SOCCER_OK) {
        L.count = io.count; L.prob = io.prob; L.next = io.next; L.reward = io.reward; L.done = io.done;
        L.tuple_of = d_tuple_of; L.lut = h->P.lut; L.offset = d_off; L.nS = nS;
        e = hipMemcpyAsync(d_tuple_of, tuple_of.data(), (size_t)nS * sizeof(int32_t), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_off, 0, off.size() * sizeof(int32_t), h->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(enumerate_kernel, dim3((unsigned)((keys + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, h->P, io);
            hipLaunchKernelGGL(minimax_lists_kernel<false>, dim3((unsigned)((nkeys + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, L);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(off.data(), d_off, off.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) rc = fail(h, SOCCER_E_HIP, "minimax list construction failed: %s", hipGetErrorString(e));
    }
    if (rc == SOCCER_OK) {
        for (size_t k = 0; k < nkeys; ++k) off[k + 1] += off[k];                 // padded lengths -> offsets
        rc = h->mm_bufs.alloc(h, (size_t)off[nkeys], &d_list);
    }
    if (rc == SOCCER_OK) {
        L.list = d_list;
        e = hipMemcpyAsync(d_off, off.data(), off.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(minimax_lists_kernel<true>, dim3((unsigned)((nkeys + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, L);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) rc = fail(h, SOCCER_E_HIP, "minimax list construction failed: %s", hipGetErrorString(e));
    }
    tmp.clear();                                // before the solver's buffers are allocated
    MinimaxIO mm{};
    if (!rc) rc = h->mm_bufs.alloc(h, (size_t)nS, &h->mm_V[0]);
    if (!rc) rc = h->mm_bufs.alloc(h, (size_t)nS, &h->mm_V[1]);
    if (!rc) rc = h->mm_bufs.alloc(h, (size_t)nS * 25, &mm.Q);
    if (!rc) rc = h->mm_bufs.alloc(h, (size_t)nS * 5, &mm.pi_a);
    if (!rc) rc = h->mm_bufs.alloc(h, (size_t)nS * 5, &mm.pi_b);
    if (!rc) rc = h->mm_bufs.alloc(h, (size_t)kMinimaxBatch + 1, &h->mm_words);
    if (rc) { h->mm_bufs.clear(); return rc; }
    mm.offset = d_off; mm.list = d_list; mm.nS = nS;
    h->mm = mm;
    h->mm_bufs.ready = true;
    return SOCCER_OK;
}

static int minimax_check(soccer_handle* h, const char* what, double gamma) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "%s during graph capture", what);
    if (h->P.policy_a != nullptr || h->P.policy_b != nullptr)
        return fail(h, SOCCER_E_INVALID, "%s needs a two-player handle: neither side may have a fixed policy (soccer_set_policy)", what);
    if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(h, SOCCER_E_INVALID, "discount_factor must be in [0, 1]");
    return SOCCER_OK;
}

// after every argument is checked: the device and the cached lists
static int minimax_prepare(soccer_handle* h) {
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return build_minimax(h);
}

// one sweep: V_in -> V_out (device buffers of the handle), Q and the strategies into the handle's buffers
static void minimax_launch(soccer_handle* h, double gamma, double theta, const double* V_in, double* V_out,
                           unsigned long long* delta, const unsigned long long* prev) {
    MinimaxIO io = h->mm;
    io.V = V_in; io.V_out = V_out; io.delta = delta; io.prev = prev; io.gamma = gamma; io.theta = theta;
    const unsigned grid = (unsigned)((io.nS + kMinimaxWaves - 1) / kMinimaxWaves);
    hipLaunchKernelGGL(minimax_sweep_kernel, dim3(grid), dim3(kMinimaxBlock), 0, h->stream, io);
}

static int minimax_outputs(soccer_handle* h, const double* V_dev, double* V, double* Q, double* pi_a, double* pi_b) {
    const size_t nS = (size_t)h->mm.nS;
    if (V) HIP_TRY(h, hipMemcpyAsync(V, V_dev, nS * 8, hipMemcpyDeviceToHost, h->stream));
    if (Q) HIP_TRY(h, hipMemcpyAsync(Q, h->mm.Q, nS * 200, hipMemcpyDeviceToHost, h->stream));
    if (pi_a) HIP_TRY(h, hipMemcpyAsync(pi_a, h->mm.pi_a, nS * 40, hipMemcpyDeviceToHost, h->stream));
    if (pi_b) HIP_TRY(h, hipMemcpyAsync(pi_b, h->mm.pi_b, nS * 40, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SOCCER_OK;
}

extern "C" int soccer_solve_matrix_games(soccer_handle* h, int64_t n_games, const double* A, double* value, double* x, double* y) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_solve_matrix_games during graph capture");
    if (n_games < 0) return fail(h, SOCCER_E_INVALID, "n_games must be >= 0");
    if (n_games > 0 && !A) return fail(h, SOCCER_E_INVALID, "A is NULL");
    if (n_games == 0) return SOCCER_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t n = (size_t)n_games;
    OwnedBufs tmp("the matrix games");                                  // freed on every way out
    double* d_A = nullptr; double* d_out[3] = {nullptr, nullptr, nullptr};            // value, x, y
    const size_t doubles[3] = {n, n * 5, n * 5};
    int rc = tmp.alloc(h, n * 25, &d_A);
    for (int i = 0; i < 3 && !rc; ++i) rc = tmp.alloc(h, doubles[i], &d_out[i]);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(d_A, A, n * 200, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        const unsigned grid = (unsigned)((n + kGamesBlock - 1) / kGamesBlock);
        hipLaunchKernelGGL(games_kernel, dim3(grid), dim3(kGamesBlock), 0, h->stream, static_cast<const double*>(d_A), (long long)n,
                           d_out[0], d_out[1], d_out[2]);
        e = hipGetLastError();
    }
    double* dst[3] = {value, x, y};
    for (int i = 0; i < 3 && e == hipSuccess; ++i) if (dst[i]) e = hipMemcpyAsync(dst[i], d_out[i], doubles[i] * 8, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, SOCCER_E_HIP, "soccer_solve_matrix_games failed: %s", hipGetErrorString(e));
    return SOCCER_OK;
}

extern "C" int soccer_minimax_backup(soccer_handle* h, double discount_factor, const double* V, double* V_out, double* Q,
                                     double* pi_a, double* pi_b) {
    if (int rc = minimax_check(h, "soccer_minimax_backup", discount_factor)) return rc;
    if (!V) return fail(h, SOCCER_E_INVALID, "V is NULL");
    if (int rc = minimax_prepare(h)) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->mm_V[0], V, (size_t)h->mm.nS * 8, hipMemcpyHostToDevice, h->stream));
    minimax_launch(h, discount_factor, 0.0, h->mm_V[0], h->mm_V[1], nullptr, nullptr);
    HIP_TRY(h, hipGetLastError());
    return minimax_outputs(h, h->mm_V[1], V_out, Q, pi_a, pi_b);
}

extern "C" int soccer_minimax_value_iteration(soccer_handle* h, double theta, double discount_factor, int32_t max_sweeps,
                                              double* V, double* Q, double* pi_a, double* pi_b, int32_t* iterations) {
    if (int rc = minimax_check(h, "soccer_minimax_value_iteration", discount_factor)) return rc;
    if (max_sweeps < 1) return fail(h, SOCCER_E_INVALID, "max_sweeps must be >= 1");
    if (!(theta >= 0.0)) return fail(h, SOCCER_E_INVALID, "theta must be >= 0");
    if (int rc = minimax_prepare(h)) return rc;
    const int nS = h->mm.nS;
    HIP_TRY(h, hipMemsetAsync(h->mm_V[0], 0, (size_t)nS * 8, h->stream));                  // V_0 = 0
    // words[0] is the sweep before the batch's first: +inf (never converged) before sweep 1
    unsigned long long words[kMinimaxBatch + 1];
    const double inf = __builtin_huge_val();
    std::memcpy(&words[0], &inf, 8);
    int32_t k0 = 1, done_at = 0;                                                         // k0: first sweep of the batch
    while (k0 <= max_sweeps && !done_at) {
        const int nb = (int)std::min<int64_t>(kMinimaxBatch, (int64_t)max_sweeps - k0 + 1);
        for (int j = 1; j <= kMinimaxBatch; ++j) words[j] = 0ull;
        HIP_TRY(h, hipMemcpyAsync(h->mm_words, words, sizeof words, hipMemcpyHostToDevice, h->stream));
        for (int j = 1; j <= nb; ++j) {
            const int32_t k = k0 + j - 1;
            minimax_launch(h, discount_factor, theta, h->mm_V[(k - 1) & 1], h->mm_V[k & 1], h->mm_words + j, h->mm_words + j - 1);
        }
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(words, h->mm_words, sizeof words, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (int j = 1; j <= nb && !done_at; ++j) {
            double d; std::memcpy(&d, &words[j], 8);
            if (d < theta) done_at = k0 + j - 1;
        }
        words[0] = words[nb];
        k0 += nb;
    }
    const int32_t k = done_at ? done_at : max_sweeps;
    if (int rc = minimax_outputs(h, h->mm_V[k & 1], V, Q, pi_a, pi_b)) return rc;
    if (iterations) *iterations = k;
    if (!done_at) return fail(h, SOCCER_E_STATE, "soccer_minimax_value_iteration stopped after max_sweeps = %d sweeps without converging", max_sweeps);
    return SOCCER_OK;
}

// ------------------------------------------------------------------------------------------------
// best responses to mixed policies and the value of a pair of them, for a batch of policies at once (two-player handles).
// The lists are build_minimax's; a sweep is one launch of response_sweep_kernel over all (policy, state) pairs, and every
// policy has its own word per sweep, so it stops at its own sweep and its result does not depend on what shares the batch.
static int response_buffers(soccer_handle* h, int n, bool pairs) {
    if (n <= h->br_cap && (!pairs || h->br_pairs)) return SOCCER_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t cap = (size_t)std::max(n, h->br_cap), rows = cap * (size_t)h->mm.nS;
    pairs = pairs || h->br_pairs;
    h->br_bufs.clear();
    h->br_cap = 0; h->br_pairs = false;
    int rc = h->br_bufs.alloc(h, rows * 5, &h->br_pol[0]);
    if (!rc && pairs) rc = h->br_bufs.alloc(h, rows * 5, &h->br_pol[1]);
    if (!rc) rc = h->br_bufs.alloc(h, rows, &h->br_V[0]);
    if (!rc) rc = h->br_bufs.alloc(h, rows, &h->br_V[1]);
    if (!rc) rc = h->br_bufs.alloc(h, rows * 5, &h->br_Qr);
    if (!rc) rc = h->br_bufs.alloc(h, rows, &h->br_arg);
    if (!rc) rc = h->br_bufs.alloc(h, cap * (kMinimaxBatch + 1), &h->br_words);
    if (rc) { h->br_bufs.clear(); return rc; }
    h->br_cap = (int)cap; h->br_pairs = pairs;
    return SOCCER_OK;
}

// soccer_minimax_q_create's check of opponent_policy, on every live row of every policy (row 0 is not read)
static int response_rows(soccer_handle* h, const char* what, const char* name, int n, const double* pol) {
    if (!pol) return fail(h, SOCCER_E_INVALID, "%s: %s is NULL", what, name);
    const int nS = h->rules.nS;
    for (int i = 0; i < n; ++i) for (int s = 1; s < nS; ++s) {
        const double* p = pol + ((size_t)i * nS + s) * 5;
        double sum = 0.0;
        for (int k = 0; k < 5; ++k) {
            if (!(p[k] >= 0.0)) return fail(h, SOCCER_E_INVALID, "%s: %s[%d][%d][%d] is negative or not a number", what, name, i, s, k);
            sum = sum + p[k];
        }
        if (!(std::fabs(sum - 1.0) <= 1e-8 + 1e-5)) return fail(h, SOCCER_E_INVALID, "%s: %s[%d][%d] does not sum to 1", what, name, i, s);
    }
    return SOCCER_OK;
}

// the caller's policies into a device block, row 0 of each as zeros
static int response_upload(soccer_handle* h, double* dst, const double* pol, int n, hipMemcpyKind kind = hipMemcpyHostToDevice) {
    const size_t pitch = (size_t)h->mm.nS * 40;
    HIP_TRY(h, hipMemcpyAsync(dst, pol, (size_t)n * pitch, kind, h->stream));
    HIP_TRY(h, hipMemset2DAsync(dst, pitch, 0, 40, (size_t)n, h->stream));
    return SOCCER_OK;
}

static int response_solve(soccer_handle* h, const char* what, int mode, int32_t n, const double* x, const double* y, double theta,
                          double gamma, int32_t max_sweeps, double* V, double* Qr, int32_t* br, int32_t* iterations) {
    if (int rc = minimax_check(h, what, gamma)) return rc;
    if (n < 1 || n > SOCCER_BR_MAX_POLICIES)
        return fail(h, SOCCER_E_INVALID, "%s: the number of policies must be 1 .. %d, not %d", what, SOCCER_BR_MAX_POLICIES, n);
    if (max_sweeps < 1) return fail(h, SOCCER_E_INVALID, "max_sweeps must be >= 1");
    if (!(theta >= 0.0)) return fail(h, SOCCER_E_INVALID, "theta must be >= 0");
    if (mode != kRespondA) if (int rc = response_rows(h, what, mode == kEvalPair ? "pi_a" : "policy", n, x)) return rc;
    if (mode != kRespondB) if (int rc = response_rows(h, what, mode == kEvalPair ? "pi_b" : "policy", n, y)) return rc;
    if (int rc = minimax_prepare(h)) return rc;
    if (int rc = response_buffers(h, n, mode == kEvalPair)) return rc;
    const int nS = h->mm.nS;
    constexpr int kWords = kMinimaxBatch + 1;
    ResponseIO io{};
    io.mm = h->mm; io.mm.gamma = gamma; io.mm.theta = theta;
    io.Qr = h->br_Qr; io.br = h->br_arg; io.word_stride = kWords;
    if (mode != kRespondA) { io.x = h->br_pol[0]; if (int rc = response_upload(h, h->br_pol[0], x, n)) return rc; }
    if (mode != kRespondB) {
        double* d = h->br_pol[mode == kEvalPair ? 1 : 0];
        io.y = d;
        if (int rc = response_upload(h, d, y, n)) return rc;
    }
    HIP_TRY(h, hipMemsetAsync(h->br_V[0], 0, (size_t)n * nS * 8, h->stream));                // V_0 = 0
    // words[i][0] is the sweep before the batch's first: +inf (never converged) before sweep 1
    std::vector<unsigned long long> words((size_t)n * kWords, 0ull);
    std::vector<int32_t> done_at((size_t)n, 0);
    const double inf = __builtin_huge_val();
    for (int i = 0; i < n; ++i) std::memcpy(&words[(size_t)i * kWords], &inf, 8);
    const dim3 grid((unsigned)((nS + kResponseStates - 1) / kResponseStates), (unsigned)n);
    int32_t k0 = 1, open = n;                                                              // k0: first sweep of the batch
    while (k0 <= max_sweeps && open) {
        const int nb = (int)std::min<int64_t>(kMinimaxBatch, (int64_t)max_sweeps - k0 + 1);
        for (int i = 0; i < n; ++i) for (int j = 1; j < kWords; ++j) words[(size_t)i * kWords + j] = 0ull;
        HIP_TRY(h, hipMemcpyAsync(h->br_words, words.data(), words.size() * 8, hipMemcpyHostToDevice, h->stream));
        for (int j = 1; j <= nb; ++j) {
            const int32_t k = k0 + j - 1;
            io.V = h->br_V[(k - 1) & 1]; io.V_out = h->br_V[k & 1]; io.delta = h->br_words + j; io.prev = h->br_words + j - 1;
            if (mode == kRespondB) hipLaunchKernelGGL(response_sweep_kernel<kRespondB>, grid, dim3(kMinimaxBlock), 0, h->stream, io);
            else if (mode == kRespondA) hipLaunchKernelGGL(response_sweep_kernel<kRespondA>, grid, dim3(kMinimaxBlock), 0, h->stream, io);
            else hipLaunchKernelGGL(response_sweep_kernel<kEvalPair>, grid, dim3(kMinimaxBlock), 0, h->stream, io);
        }
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(words.data(), h->br_words, words.size() * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (int i = 0; i < n; ++i) {
            unsigned long long* w = &words[(size_t)i * kWords];
            for (int j = 1; j <= nb && !done_at[i]; ++j) {
                double d; std::memcpy(&d, &w[j], 8);
                if (d < theta) { done_at[i] = k0 + j - 1; --open; }
            }
            w[0] = w[nb];                       // a policy that has converged keeps a word below theta: its blocks go on returning
        }
        k0 += nb;
    }
    int first_open = -1;
    for (int i = 0; i < n; ++i) {
        const int32_t k = done_at[i] ? done_at[i] : max_sweeps;
        if (!done_at[i] && first_open < 0) first_open = i;
        if (iterations) iterations[i] = k;
        if (V) HIP_TRY(h, hipMemcpyAsync(V + (size_t)i * nS, h->br_V[k & 1] + (size_t)i * nS, (size_t)nS * 8, hipMemcpyDeviceToHost, h->stream));
    }
    if (Qr) HIP_TRY(h, hipMemcpyAsync(Qr, h->br_Qr, (size_t)n * nS * 40, hipMemcpyDeviceToHost, h->stream));
    if (br) HIP_TRY(h, hipMemcpyAsync(br, h->br_arg, (size_t)n * nS * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (open) return fail(h, SOCCER_E_STATE, "%s: %d of %d policies had not converged after max_sweeps = %d sweeps (the first: policy %d)",
                          what, open, n, max_sweeps, first_open);
    return SOCCER_OK;
}

extern "C" int soccer_best_response(soccer_handle* h, int32_t player, int32_t n_policies, const double* policy, double theta,
                                    double discount_factor, int32_t max_sweeps, double* V, double* Qr, int32_t* br, int32_t* iterations) {
    if (h && player != 0 && player != 1) return fail(h, SOCCER_E_INVALID, "soccer_best_response: player must be 0 (the policy is A's) or 1 (B's)");
    const bool a_fixed = player == 0;
    return response_solve(h, "soccer_best_response", a_fixed ? kRespondB : kRespondA, n_policies, a_fixed ? policy : nullptr,
                          a_fixed ? nullptr : policy, theta, discount_factor, max_sweeps, V, Qr, br, iterations);
}

extern "C" int soccer_evaluate_policies(soccer_handle* h, int32_t n_pairs, const double* pi_a, const double* pi_b, double theta,
                                        double discount_factor, int32_t max_sweeps, double* V, int32_t* iterations) {
    return response_solve(h, "soccer_evaluate_policies", kEvalPair, n_pairs, pi_a, pi_b, theta, discount_factor, max_sweeps,
                          V, nullptr, nullptr, iterations);
}

// ------------------------------------------------------------------------------------------------
// cross-play: player A's value of every pair (pi_a[i], pi_b[j]) of two sets of mixed policies.  Each pair is
// soccer_evaluate_policies' iteration, solved to the bits it has alone; the work is laid out the other way round (a lane owns
// a pair, cross_sweep_kernel), the policies are uploaded once, a matrix larger than a pass is solved pass after pass over the
// same buffers, and the stopping sweeps are found on the device: a batch of sweeps costs the host one 4-byte read.
static int cross_buffers(soccer_handle* h, int policies, int stride, bool values) {
    if (policies <= h->cx_policies && stride <= h->cx_stride && (!values || h->cx_has_values)) return SOCCER_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    policies = std::max(policies, h->cx_policies); stride = std::max(stride, h->cx_stride); values = values || h->cx_has_values;
    h->cx_bufs.clear();
    h->cx_policies = 0; h->cx_stride = 0; h->cx_has_values = false;
    const size_t nS = (size_t)h->mm.nS, cells = nS * (size_t)stride;
    int rc = h->cx_bufs.alloc(h, (size_t)policies * nS * 5, &h->cx_pol);
    if (!rc) rc = h->cx_bufs.alloc(h, cells, &h->cx_V[0]);
    if (!rc) rc = h->cx_bufs.alloc(h, cells, &h->cx_V[1]);
    if (!rc) rc = h->cx_bufs.alloc(h, (size_t)stride * (kMinimaxBatch + 1), &h->cx_words);
    if (!rc) rc = h->cx_bufs.alloc(h, (size_t)stride, &h->cx_done);
    if (!rc) rc = h->cx_bufs.alloc(h, (size_t)stride, &h->cx_iter);
    if (!rc) rc = h->cx_bufs.alloc(h, (size_t)stride, &h->cx_payoff);
    if (!rc) rc = h->cx_bufs.alloc(h, (size_t)1, &h->cx_open);
    if (!rc && values) rc = h->cx_bufs.alloc(h, cells, &h->cx_values);
    if (rc) { h->cx_bufs.clear(); return rc; }
    h->cx_policies = policies; h->cx_stride = stride; h->cx_has_values = values;
    return SOCCER_OK;
}

// One pass of a solve whose pairs stop one by one (soccer_cross_play, soccer_occupancy, soccer_policy_gradient): both buffers
// cleared, then batches of sweeps until every pair has stopped or max_sweeps is reached, the stopping sweeps found on the
// device (cross_batch_kernel) and read back as one count per batch.  sweep(k, in, out, delta, prev) launches sweep k;
// open_left (may be NULL) takes the number of pairs still open at the end.
struct PassBufs {
    double* buf[2];                         // [nS][stride] double-buffered across sweeps
    unsigned long long* words;              // [kMinimaxBatch + 1][stride]
    int32_t* done;                          // [stride]
    int32_t* open;
    int stride;
};

template <class Sweep>
static int solve_pass(soccer_handle* h, const PassBufs& B, int nS, int pairs, double theta, int32_t max_sweeps, Sweep sweep, int32_t* open_left) {
    const size_t stride = (size_t)B.stride;
    const unsigned pair_blocks = (unsigned)((pairs + kCrossBlock - 1) / kCrossBlock);
    CrossBatchIO bio{};
    bio.words = B.words; bio.done_at = B.done; bio.open = B.open; bio.theta = theta; bio.stride = B.stride; bio.n_words = kMinimaxBatch + 1;
    bio.pairs = pairs;
    HIP_TRY(h, hipMemsetAsync(B.buf[0], 0, (size_t)nS * stride * 8, h->stream));           // the iterate before sweep 1 is 0
    HIP_TRY(h, hipMemsetAsync(B.buf[1], 0, (size_t)nS * stride * 8, h->stream));
    HIP_TRY(h, hipMemsetAsync(B.open, 0, sizeof(int32_t), h->stream));
    bio.k0 = 0; bio.nb = 0;
    hipLaunchKernelGGL(cross_batch_kernel, dim3(pair_blocks), dim3(kCrossBlock), 0, h->stream, bio);
    int32_t k0 = 1, open = pairs;                                                          // k0: first sweep of the batch
    while (k0 <= max_sweeps && open) {
        const int nb = (int)std::min<int64_t>(kMinimaxBatch, (int64_t)max_sweeps - k0 + 1);
        for (int j = 1; j <= nb; ++j) {
            const int32_t k = k0 + j - 1;
            sweep(k, B.buf[(k - 1) & 1], B.buf[k & 1], B.words + (size_t)j * stride, B.words + (size_t)(j - 1) * stride);
        }
        HIP_TRY(h, hipMemsetAsync(B.open, 0, sizeof(int32_t), h->stream));
        bio.k0 = k0; bio.nb = nb;
        hipLaunchKernelGGL(cross_batch_kernel, dim3(pair_blocks), dim3(kCrossBlock), 0, h->stream, bio);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(&open, B.open, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        k0 += nb;
    }
    if (open_left) *open_left = open;
    return SOCCER_OK;
}

// cross-play's pass over device-resident policies: io holds everything but the buffers of a sweep
static int cross_solve_pass(soccer_handle* h, CrossIO io, const PassBufs& B, int32_t max_sweeps, int32_t* open_left) {
    const dim3 grid((unsigned)((io.nS + kCrossWaves - 1) / kCrossWaves), (unsigned)((io.pairs + 63) / 64));
    return solve_pass(h, B, io.nS, io.pairs, io.theta, max_sweeps,
                      [&](int32_t, const double* in, double* out, unsigned long long* delta, const unsigned long long* prev) {
                          io.V = in; io.V_out = out; io.delta = delta; io.prev = prev;
                          hipLaunchKernelGGL(cross_sweep_kernel, grid, dim3(kCrossBlock), 0, h->stream, io);
                      }, open_left);
}

// the occupancy's, likewise (the policies transposed: occupancy_transposed)
static int occupancy_solve_pass(soccer_handle* h, OccupancyIO io, const PassBufs& B, int32_t max_sweeps, int32_t* open_left) {
    const dim3 grid((unsigned)((io.nS + kCrossWaves - 1) / kCrossWaves), (unsigned)((io.pairs + 63) / 64));
    return solve_pass(h, B, io.nS, io.pairs, io.theta, max_sweeps,
                      [&](int32_t, const double* in, double* out, unsigned long long* delta, const unsigned long long* prev) {
                          io.D = in; io.D_out = out; io.delta = delta; io.prev = prev;
                          hipLaunchKernelGGL(occupancy_sweep_kernel, grid, dim3(kCrossBlock), 0, h->stream, io);
                      }, open_left);
}

extern "C" int soccer_cross_play(soccer_handle* h, int32_t n_a, const double* pi_a, int32_t n_b, const double* pi_b, double theta,
                                 double discount_factor, int32_t max_sweeps, int32_t pairs_per_pass, double* payoff, double* V,
                                 int32_t* iterations) {
    const char* what = "soccer_cross_play";
    if (int rc = minimax_check(h, what, discount_factor)) return rc;
    if (n_a < 1 || n_a > SOCCER_CROSS_MAX_POLICIES || n_b < 1 || n_b > SOCCER_CROSS_MAX_POLICIES)
        return fail(h, SOCCER_E_INVALID, "%s: the number of policies of each player must be 1 .. %d, not %d and %d", what,
                    SOCCER_CROSS_MAX_POLICIES, n_a, n_b);
    if (max_sweeps < 1) return fail(h, SOCCER_E_INVALID, "max_sweeps must be >= 1");
    if (!(theta >= 0.0)) return fail(h, SOCCER_E_INVALID, "theta must be >= 0");
    if (pairs_per_pass < 0 || pairs_per_pass % 64)
        return fail(h, SOCCER_E_INVALID, "%s: pairs_per_pass must be 0 (the library chooses) or a positive multiple of 64, not %d", what, pairs_per_pass);
    if (int rc = response_rows(h, what, "pi_a", n_a, pi_a)) return rc;
    if (int rc = response_rows(h, what, "pi_b", n_b, pi_b)) return rc;
    if (int rc = minimax_prepare(h)) return rc;
    const int nS = h->mm.nS;
    const int total = n_a * n_b, total64 = (total + 63) / 64 * 64;
    // the library's choice: the two V buffers of a pass, 2 * nS * pairs * 8 bytes, stay at or under 1 GiB
    int per_pass = pairs_per_pass ? pairs_per_pass : std::max(64, (int)(((size_t)1 << 30) / ((size_t)16 * nS) / 64 * 64));
    per_pass = std::min(per_pass, total64);
    if (int rc = cross_buffers(h, n_a + n_b, per_pass, V != nullptr)) return rc;
    const int stride = h->cx_stride;                                    // (what an earlier, larger pass left: no result depends on it)
    double* d_x = h->cx_pol; double* d_y = h->cx_pol + (size_t)n_a * nS * 5;
    if (int rc = response_upload(h, d_x, pi_a, n_a)) return rc;
    if (int rc = response_upload(h, d_y, pi_b, n_b)) return rc;
    CrossIO io{};
    io.offset = h->mm.offset; io.list = h->mm.list; io.x = d_x; io.y = d_y; io.gamma = discount_factor; io.theta = theta;
    io.nS = nS; io.n_b = n_b; io.stride = stride; io.last = total - 1;
    const PassBufs pass{{h->cx_V[0], h->cx_V[1]}, h->cx_words, h->cx_done, h->cx_open, stride};
    CrossFinishIO fio{};
    fio.V[0] = h->cx_V[0]; fio.V[1] = h->cx_V[1]; fio.done_at = h->cx_done; fio.payoff = h->cx_payoff; fio.iterations = h->cx_iter;
    fio.values = h->cx_values; fio.n_isd = h->rules.n_isd; fio.nS = nS; fio.stride = stride; fio.max_sweeps = max_sweeps;
    for (int i = 0; i < h->rules.n_isd; ++i) fio.isd[i] = (int32_t)h->rules.isd_obs[i];
    int64_t open_total = 0;
    for (int first = 0; first < total; first += per_pass) {
        const int pairs = std::min(per_pass, total - first);
        const unsigned pair_blocks = (unsigned)((pairs + kCrossBlock - 1) / kCrossBlock);
        io.first = first; io.pairs = pairs; fio.pairs = pairs;
        int32_t open = 0;
        if (int rc = cross_solve_pass(h, io, pass, max_sweeps, &open)) return rc;          // V_0 = 0
        open_total += open;
        hipLaunchKernelGGL(cross_finish_kernel, dim3(pair_blocks), dim3(kCrossBlock), 0, h->stream, fio);
        if (V) hipLaunchKernelGGL(cross_values_kernel, dim3((unsigned)((pairs + 63) / 64), (unsigned)((nS + 63) / 64)), dim3(kCrossBlock), 0, h->stream, fio);
        HIP_TRY(h, hipGetLastError());
        if (payoff) HIP_TRY(h, hipMemcpyAsync(payoff + first, h->cx_payoff, (size_t)pairs * 8, hipMemcpyDeviceToHost, h->stream));
        if (iterations) HIP_TRY(h, hipMemcpyAsync(iterations + first, h->cx_iter, (size_t)pairs * 4, hipMemcpyDeviceToHost, h->stream));
        if (V) HIP_TRY(h, hipMemcpyAsync(V + (size_t)first * nS, h->cx_values, (size_t)pairs * nS * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if (open_total) return fail(h, SOCCER_E_STATE, "%s: %lld of %d pairs had not converged after max_sweeps = %d sweeps", what,
                                (long long)open_total, total, max_sweeps);
    return SOCCER_OK;
}

// ------------------------------------------------------------------------------------------------
// match outcomes: for every pair (pi_a[i], pi_b[j]) the probability that A, and that B, scores the goal that ends the game,
// and the expected number of steps it lasts, when every step is followed by another with probability continue_prob.
// cross-play's host scheme (passes, batches of sweeps, the stopping sweeps found on the device) over three-channel buffers:
// a sweep is one launch of match_sweep_kernel, which reads every list entry once for the three sums.
static int match_buffers(soccer_handle* h, int policies, int stride, bool values) {
    if (policies <= h->mo_policies && stride <= h->mo_stride && (!values || h->mo_has_values)) return SOCCER_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    policies = std::max(policies, h->mo_policies); stride = std::max(stride, h->mo_stride); values = values || h->mo_has_values;
    h->mo_bufs.clear();
    h->mo_policies = 0; h->mo_stride = 0; h->mo_has_values = false;
    const size_t nS = (size_t)h->mm.nS, cells = kMatchChannels * nS * (size_t)stride;
    int rc = h->mo_bufs.alloc(h, (size_t)policies * nS * 5, &h->mo_pol);
    if (!rc) rc = h->mo_bufs.alloc(h, cells, &h->mo_V[0]);
    if (!rc) rc = h->mo_bufs.alloc(h, cells, &h->mo_V[1]);
    if (!rc) rc = h->mo_bufs.alloc(h, (size_t)stride * (kMinimaxBatch + 1), &h->mo_words);
    if (!rc) rc = h->mo_bufs.alloc(h, (size_t)stride, &h->mo_done);
    if (!rc) rc = h->mo_bufs.alloc(h, (size_t)stride, &h->mo_iter);
    if (!rc) rc = h->mo_bufs.alloc(h, (size_t)kMatchChannels * stride, &h->mo_kickoff);
    if (!rc) rc = h->mo_bufs.alloc(h, (size_t)1, &h->mo_open);
    if (!rc && values) rc = h->mo_bufs.alloc(h, cells, &h->mo_values);
    if (rc) { h->mo_bufs.clear(); return rc; }
    h->mo_policies = policies; h->mo_stride = stride; h->mo_has_values = values;
    return SOCCER_OK;
}

extern "C" int soccer_match_outcomes(soccer_handle* h, int32_t n_a, const double* pi_a, int32_t n_b, const double* pi_b, double theta,
                                     double continue_prob, int32_t max_sweeps, int32_t pairs_per_pass, double* win_a, double* win_b,
                                     double* length, double* values, int32_t* iterations) {
    const char* what = "soccer_match_outcomes";
    if (int rc = minimax_check(h, what, 0.0)) return rc;
    if (!(continue_prob >= 0.0 && continue_prob <= 1.0)) return fail(h, SOCCER_E_INVALID, "continue_prob must be in [0, 1]");
    if (n_a < 1 || n_a > SOCCER_CROSS_MAX_POLICIES || n_b < 1 || n_b > SOCCER_CROSS_MAX_POLICIES)
        return fail(h, SOCCER_E_INVALID, "%s: the number of policies of each player must be 1 .. %d, not %d and %d", what,
                    SOCCER_CROSS_MAX_POLICIES, n_a, n_b);
    if (max_sweeps < 1) return fail(h, SOCCER_E_INVALID, "max_sweeps must be >= 1");
    if (!(theta >= 0.0)) return fail(h, SOCCER_E_INVALID, "theta must be >= 0");
    if (pairs_per_pass < 0 || pairs_per_pass % 64)
        return fail(h, SOCCER_E_INVALID, "%s: pairs_per_pass must be 0 (the library chooses) or a positive multiple of 64, not %d", what, pairs_per_pass);
    if (int rc = response_rows(h, what, "pi_a", n_a, pi_a)) return rc;
    if (int rc = response_rows(h, what, "pi_b", n_b, pi_b)) return rc;
    if (int rc = minimax_prepare(h)) return rc;
    const int nS = h->mm.nS;
    const int total = n_a * n_b, total64 = (total + 63) / 64 * 64;
    // the library's choice: the two three-channel buffers of a pass, 2 * 3 * nS * pairs * 8 bytes, stay at or under 1 GiB
    int per_pass = pairs_per_pass ? pairs_per_pass : std::max(64, (int)(((size_t)1 << 30) / ((size_t)16 * kMatchChannels * nS) / 64 * 64));
    per_pass = std::min(per_pass, total64);
    if (int rc = match_buffers(h, n_a + n_b, per_pass, values != nullptr)) return rc;
    const int stride = h->mo_stride;                                    // (what an earlier, larger pass left: no result depends on it)
    const size_t cells = (size_t)kMatchChannels * nS * stride;
    double* d_x = h->mo_pol; double* d_y = h->mo_pol + (size_t)n_a * nS * 5;
    if (int rc = response_upload(h, d_x, pi_a, n_a)) return rc;
    if (int rc = response_upload(h, d_y, pi_b, n_b)) return rc;
    constexpr int kWords = kMinimaxBatch + 1;
    CrossIO io{};
    io.offset = h->mm.offset; io.list = h->mm.list; io.x = d_x; io.y = d_y; io.gamma = continue_prob; io.theta = theta;
    io.nS = nS; io.n_b = n_b; io.stride = stride; io.last = total - 1;
    CrossBatchIO bio{};
    bio.words = h->mo_words; bio.done_at = h->mo_done; bio.open = h->mo_open; bio.theta = theta; bio.stride = stride; bio.n_words = kWords;
    MatchFinishIO fio{};
    fio.V[0] = h->mo_V[0]; fio.V[1] = h->mo_V[1]; fio.done_at = h->mo_done; fio.kickoff = h->mo_kickoff; fio.iterations = h->mo_iter;
    fio.values = h->mo_values; fio.n_isd = h->rules.n_isd; fio.nS = nS; fio.stride = stride; fio.max_sweeps = max_sweeps;
    for (int i = 0; i < h->rules.n_isd; ++i) fio.isd[i] = (int32_t)h->rules.isd_obs[i];
    double* const outs[kMatchChannels] = {win_a, win_b, length};
    int64_t open_total = 0;
    for (int first = 0; first < total; first += per_pass) {
        const int pairs = std::min(per_pass, total - first);
        const unsigned pair_blocks = (unsigned)((pairs + kCrossBlock - 1) / kCrossBlock);
        io.first = first; io.pairs = pairs; bio.pairs = pairs; fio.pairs = pairs;
        HIP_TRY(h, hipMemsetAsync(h->mo_V[0], 0, cells * 8, h->stream));                     // W_A = W_B = L = 0
        HIP_TRY(h, hipMemsetAsync(h->mo_V[1], 0, cells * 8, h->stream));
        HIP_TRY(h, hipMemsetAsync(h->mo_open, 0, sizeof(int32_t), h->stream));
        bio.k0 = 0; bio.nb = 0;
        hipLaunchKernelGGL(cross_batch_kernel, dim3(pair_blocks), dim3(kCrossBlock), 0, h->stream, bio);
        const dim3 grid((unsigned)((nS + kCrossWaves - 1) / kCrossWaves), (unsigned)((pairs + 63) / 64));
        int32_t k0 = 1, open = pairs;                                                          // k0: first sweep of the batch
        while (k0 <= max_sweeps && open) {
            const int nb = (int)std::min<int64_t>(kMinimaxBatch, (int64_t)max_sweeps - k0 + 1);
            for (int j = 1; j <= nb; ++j) {
                const int32_t k = k0 + j - 1;
                io.V = h->mo_V[(k - 1) & 1]; io.V_out = h->mo_V[k & 1];
                io.delta = h->mo_words + (size_t)j * stride; io.prev = h->mo_words + (size_t)(j - 1) * stride;
                hipLaunchKernelGGL(match_sweep_kernel, grid, dim3(kCrossBlock), 0, h->stream, io);
            }
            HIP_TRY(h, hipMemsetAsync(h->mo_open, 0, sizeof(int32_t), h->stream));
            bio.k0 = k0; bio.nb = nb;
            hipLaunchKernelGGL(cross_batch_kernel, dim3(pair_blocks), dim3(kCrossBlock), 0, h->stream, bio);
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, hipMemcpyAsync(&open, h->mo_open, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(h, hipStreamSynchronize(h->stream));
            k0 += nb;
        }
        open_total += open;
        hipLaunchKernelGGL(match_finish_kernel, dim3(pair_blocks), dim3(kCrossBlock), 0, h->stream, fio);
        if (values) hipLaunchKernelGGL(match_values_kernel, dim3((unsigned)((pairs + 63) / 64), (unsigned)((nS + 63) / 64), kMatchChannels),
                                       dim3(kCrossBlock), 0, h->stream, fio);
        HIP_TRY(h, hipGetLastError());
        for (int c = 0; c < kMatchChannels; ++c)
            if (outs[c]) HIP_TRY(h, hipMemcpyAsync(outs[c] + first, h->mo_kickoff + (size_t)c * stride, (size_t)pairs * 8, hipMemcpyDeviceToHost, h->stream));
        if (iterations) HIP_TRY(h, hipMemcpyAsync(iterations + first, h->mo_iter, (size_t)pairs * 4, hipMemcpyDeviceToHost, h->stream));
        if (values) HIP_TRY(h, hipMemcpyAsync(values + (size_t)first * kMatchChannels * nS, h->mo_values, (size_t)pairs * kMatchChannels * nS * 8,
                                              hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if (open_total) return fail(h, SOCCER_E_STATE, "%s: %lld of %d pairs had not converged after max_sweeps = %d sweeps", what,
                                (long long)open_total, total, max_sweeps);
    return SOCCER_OK;
}

// ------------------------------------------------------------------------------------------------
// state occupancy: for every pair (pi_a[i], pi_b[j]) the expected discounted number of visits to every state from kick-off,
// the dual of cross-play's value.  The sweep sums over in-lists, the two-player lists the other way round, which are built
// on the host once per handle (soccer_inlists.hpp) from a copy of the device's lists; the rest is cross-play's host scheme
// (passes, batches of sweeps, the stopping sweeps found on the device), with the policies transposed on the device once per
// call so that the per-entry policy reads of occupancy_sweep_kernel are contiguous across the lanes.
static int build_occupancy_lists(soccer_handle* h) {
    if (h->oc_lists.ready) return SOCCER_OK;
    const int nS = h->mm.nS;
    const size_t nkeys = (size_t)nS * 25;
    std::vector<int32_t> off(nkeys + 1);
    HIP_TRY(h, hipMemcpyAsync(off.data(), h->mm.offset, off.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::vector<PlanEntry> list((size_t)off[nkeys]);
    HIP_TRY(h, hipMemcpyAsync(list.data(), h->mm.list, list.size() * sizeof(PlanEntry), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::vector<int32_t> in_off; std::vector<InEntry> in_list;
    if (!build_inlists(nS, off.data(), list.data(), in_off, in_list))
        return fail(h, SOCCER_E_INVALID, "internal error: the two-player lists have an entry whose next state is not a state");
    h->oc_lists.clear();
    int rc = h->oc_lists.upload(h, in_off, &h->oc_in_offset);
    if (!rc) rc = h->oc_lists.upload(h, in_list, &h->oc_in_list);
    if (rc) { h->oc_lists.clear(); return rc; }
    h->oc_lists.ready = true;
    return SOCCER_OK;
}

static int occupancy_buffers(soccer_handle* h, int policies, int stride, bool values) {
    if (policies <= h->oc_policies && stride <= h->oc_stride && (!values || h->oc_has_values)) return SOCCER_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    policies = std::max(policies, h->oc_policies); stride = std::max(stride, h->oc_stride); values = values || h->oc_has_values;
    h->oc_bufs.clear();
    h->oc_policies = 0; h->oc_stride = 0; h->oc_has_values = false;
    const size_t nS = (size_t)h->mm.nS, cells = nS * (size_t)stride;
    int rc = h->oc_bufs.alloc(h, (size_t)policies * nS * 5, &h->oc_pol);
    if (!rc) rc = h->oc_bufs.alloc(h, (size_t)policies * nS * 5, &h->oc_polT);
    if (!rc) rc = h->oc_bufs.alloc(h, cells, &h->oc_D[0]);
    if (!rc) rc = h->oc_bufs.alloc(h, cells, &h->oc_D[1]);
    if (!rc) rc = h->oc_bufs.alloc(h, (size_t)stride * (kMinimaxBatch + 1), &h->oc_words);
    if (!rc) rc = h->oc_bufs.alloc(h, (size_t)stride, &h->oc_done);
    if (!rc) rc = h->oc_bufs.alloc(h, (size_t)stride, &h->oc_iter);
    if (!rc) rc = h->oc_bufs.alloc(h, (size_t)stride, &h->oc_length);
    if (!rc) rc = h->oc_bufs.alloc(h, (size_t)stride * SOCCER_OCC_MAX_FEATURES, &h->oc_expect);
    if (!rc) rc = h->oc_bufs.alloc(h, (size_t)SOCCER_OCC_MAX_FEATURES * nS, &h->oc_features);
    if (!rc) rc = h->oc_bufs.alloc(h, (size_t)1, &h->oc_open);
    if (!rc && values) rc = h->oc_bufs.alloc(h, cells, &h->oc_values);
    if (rc) { h->oc_bufs.clear(); return rc; }
    h->oc_policies = policies; h->oc_stride = stride; h->oc_has_values = values;
    return SOCCER_OK;
}

// both players' device-resident policies [n][nS][5] -> [nS][5][n] (the caller checks hipGetLastError)
static void occupancy_transposed(soccer_handle* h, const double* d_x, double* d_xT, int n_a, const double* d_y, double* d_yT, int n_b) {
    const size_t rows = (size_t)h->mm.nS * 5;
    for (int side = 0; side < 2; ++side) {
        OccupancyPolicyIO pio{};
        pio.pol = side ? d_y : d_x; pio.polT = side ? d_yT : d_xT; pio.n = side ? n_b : n_a; pio.rows = (int32_t)rows;
        const size_t cells = rows * (size_t)pio.n;
        hipLaunchKernelGGL(occupancy_transpose_kernel, dim3((unsigned)((cells + kCrossBlock - 1) / kCrossBlock)), dim3(kCrossBlock), 0, h->stream, pio);
    }
}

extern "C" int soccer_occupancy(soccer_handle* h, int32_t n_a, const double* pi_a, int32_t n_b, const double* pi_b, double theta,
                                double continue_prob, int32_t max_sweeps, int32_t pairs_per_pass, int32_t n_f, const double* features,
                                double* length, double* expect, double* occupancy, int32_t* iterations) {
    const char* what = "soccer_occupancy";
    if (int rc = minimax_check(h, what, 0.0)) return rc;
    if (!(continue_prob >= 0.0 && continue_prob <= 1.0)) return fail(h, SOCCER_E_INVALID, "continue_prob must be in [0, 1]");
    if (n_a < 1 || n_a > SOCCER_CROSS_MAX_POLICIES || n_b < 1 || n_b > SOCCER_CROSS_MAX_POLICIES)
        return fail(h, SOCCER_E_INVALID, "%s: the number of policies of each player must be 1 .. %d, not %d and %d", what,
                    SOCCER_CROSS_MAX_POLICIES, n_a, n_b);
    if (max_sweeps < 1) return fail(h, SOCCER_E_INVALID, "max_sweeps must be >= 1");
    if (!(theta >= 0.0)) return fail(h, SOCCER_E_INVALID, "theta must be >= 0");
    if (pairs_per_pass < 0 || pairs_per_pass % 64)
        return fail(h, SOCCER_E_INVALID, "%s: pairs_per_pass must be 0 (the library chooses) or a positive multiple of 64, not %d", what, pairs_per_pass);
    if (n_f < 0 || n_f > SOCCER_OCC_MAX_FEATURES)
        return fail(h, SOCCER_E_INVALID, "%s: the number of features must be 0 .. %d, not %d", what, SOCCER_OCC_MAX_FEATURES, n_f);
    if (n_f > 0 && !features) return fail(h, SOCCER_E_INVALID, "%s: features is NULL", what);
    if (int rc = response_rows(h, what, "pi_a", n_a, pi_a)) return rc;
    if (int rc = response_rows(h, what, "pi_b", n_b, pi_b)) return rc;
    if (int rc = minimax_prepare(h)) return rc;
    if (int rc = build_occupancy_lists(h)) return rc;
    const int nS = h->mm.nS;
    const int total = n_a * n_b, total64 = (total + 63) / 64 * 64;
    const int sums = expect ? n_f : 0;                                  // the expectations that are formed
    // the library's choice: the two D buffers of a pass, 2 * nS * pairs * 8 bytes, stay at or under 1 GiB
    int per_pass = pairs_per_pass ? pairs_per_pass : std::max(64, (int)(((size_t)1 << 30) / ((size_t)16 * nS) / 64 * 64));
    per_pass = std::min(per_pass, total64);
    if (int rc = occupancy_buffers(h, n_a + n_b, per_pass, occupancy != nullptr)) return rc;
    const int stride = h->oc_stride;                                    // (what an earlier, larger pass left: no result depends on it)
    const size_t rows = (size_t)nS * 5;
    double* d_x = h->oc_pol; double* d_y = h->oc_pol + (size_t)n_a * rows;
    double* d_xT = h->oc_polT; double* d_yT = h->oc_polT + (size_t)n_a * rows;
    if (int rc = response_upload(h, d_x, pi_a, n_a)) return rc;
    if (int rc = response_upload(h, d_y, pi_b, n_b)) return rc;
    occupancy_transposed(h, d_x, d_xT, n_a, d_y, d_yT, n_b);
    HIP_TRY(h, hipGetLastError());
    if (sums) HIP_TRY(h, hipMemcpyAsync(h->oc_features, features, (size_t)sums * nS * 8, hipMemcpyHostToDevice, h->stream));
    OccupancyIO io{};
    io.in_offset = h->oc_in_offset; io.in_list = h->oc_in_list; io.xT = d_xT; io.yT = d_yT; io.c = continue_prob; io.theta = theta;
    io.n_isd = h->rules.n_isd; io.mu = 1.0 / (double)h->rules.n_isd;
    for (int i = 0; i < h->rules.n_isd; ++i) io.isd[i] = (int32_t)h->rules.isd_obs[i];
    io.nS = nS; io.n_a = n_a; io.n_b = n_b; io.stride = stride; io.last = total - 1;
    const PassBufs pass{{h->oc_D[0], h->oc_D[1]}, h->oc_words, h->oc_done, h->oc_open, stride};
    OccupancyFinishIO fio{};
    fio.D[0] = h->oc_D[0]; fio.D[1] = h->oc_D[1]; fio.done_at = h->oc_done; fio.features = h->oc_features;
    fio.length = length ? h->oc_length : nullptr; fio.expect = h->oc_expect; fio.iterations = h->oc_iter;
    fio.nS = nS; fio.stride = stride; fio.max_sweeps = max_sweeps; fio.n_f = sums;
    CrossFinishIO vio{};                                                // cross_values_kernel's: D is laid out like cross-play's V
    vio.V[0] = h->oc_D[0]; vio.V[1] = h->oc_D[1]; vio.done_at = h->oc_done; vio.values = h->oc_values;
    vio.nS = nS; vio.stride = stride; vio.max_sweeps = max_sweeps;
    int64_t open_total = 0;
    for (int first = 0; first < total; first += per_pass) {
        const int pairs = std::min(per_pass, total - first);
        const unsigned pair_blocks = (unsigned)((pairs + kCrossBlock - 1) / kCrossBlock);
        io.first = first; io.pairs = pairs; fio.pairs = pairs; vio.pairs = pairs;
        int32_t open = 0;
        if (int rc = occupancy_solve_pass(h, io, pass, max_sweeps, &open)) return rc;      // D_0 = 0, and row 0 of both for good
        open_total += open;
        hipLaunchKernelGGL(occupancy_finish_kernel, dim3(pair_blocks, (unsigned)(1 + sums)), dim3(kCrossBlock), 0, h->stream, fio);
        if (occupancy) hipLaunchKernelGGL(cross_values_kernel, dim3((unsigned)((pairs + 63) / 64), (unsigned)((nS + 63) / 64)), dim3(kCrossBlock), 0, h->stream, vio);
        HIP_TRY(h, hipGetLastError());
        if (length) HIP_TRY(h, hipMemcpyAsync(length + first, h->oc_length, (size_t)pairs * 8, hipMemcpyDeviceToHost, h->stream));
        if (sums) HIP_TRY(h, hipMemcpyAsync(expect + (size_t)first * sums, h->oc_expect, (size_t)pairs * sums * 8, hipMemcpyDeviceToHost, h->stream));
        if (iterations) HIP_TRY(h, hipMemcpyAsync(iterations + first, h->oc_iter, (size_t)pairs * 4, hipMemcpyDeviceToHost, h->stream));
        if (occupancy) HIP_TRY(h, hipMemcpyAsync(occupancy + (size_t)first * nS, h->oc_values, (size_t)pairs * nS * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if (open_total) return fail(h, SOCCER_E_STATE, "%s: %lld of %d pairs had not converged after max_sweeps = %d sweeps", what,
                                (long long)open_total, total, max_sweeps);
    return SOCCER_OK;
}

// ------------------------------------------------------------------------------------------------
// exact policy gradients: for every pair (pi_a[i], pi_b[j]) cross-play's V and the occupancy's D with the discount as the
// continuation probability, solved pass by pass over the same pairs at one stride (a buffer family of its own), one more
// backup from every pair's final V mixed with the other side's policy (action_values_kernel), and D * Q added to each
// policy's running weighted sum in ascending order of the other side's index (gradient_reduce_kernel), carried from pass to pass.
static int gradient_buffers(soccer_handle* h, int policies, int stride, bool values) {
    if (policies <= h->pg_policies && stride <= h->pg_stride && (!values || h->pg_has_values)) return SOCCER_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    policies = std::max(policies, h->pg_policies); stride = std::max(stride, h->pg_stride); values = values || h->pg_has_values;
    h->pg_bufs.clear();
    h->pg_policies = 0; h->pg_stride = 0; h->pg_has_values = false;
    const size_t nS = (size_t)h->mm.nS, cells = nS * (size_t)stride, rows = (size_t)policies * nS;
    int rc = h->pg_bufs.alloc(h, rows * 5, &h->pg_pol);
    if (!rc) rc = h->pg_bufs.alloc(h, rows * 5, &h->pg_polT);
    for (int i = 0; i < 2 && !rc; ++i) rc = h->pg_bufs.alloc(h, cells, &h->pg_V[i]);
    for (int i = 0; i < 2 && !rc; ++i) rc = h->pg_bufs.alloc(h, cells, &h->pg_D[i]);
    if (!rc) rc = h->pg_bufs.alloc(h, cells * 10, &h->pg_Q);
    if (!rc) rc = h->pg_bufs.alloc(h, (size_t)stride * (kMinimaxBatch + 1), &h->pg_words);
    for (int i = 0; i < 2 && !rc; ++i) rc = h->pg_bufs.alloc(h, (size_t)stride, &h->pg_done[i]);
    if (!rc) rc = h->pg_bufs.alloc(h, (size_t)stride, &h->pg_iter);
    if (!rc) rc = h->pg_bufs.alloc(h, (size_t)stride, &h->pg_payoff);
    if (!rc) rc = h->pg_bufs.alloc(h, (size_t)1, &h->pg_open);
    if (!rc) rc = h->pg_bufs.alloc(h, rows * 5, &h->pg_grad);
    if (!rc) rc = h->pg_bufs.alloc(h, rows, &h->pg_reach);
    if (!rc) rc = h->pg_bufs.alloc(h, (size_t)policies, &h->pg_w);
    if (!rc && values) rc = h->pg_bufs.alloc(h, cells * 5, &h->pg_values);
    if (rc) { h->pg_bufs.clear(); return rc; }
    h->pg_policies = policies; h->pg_stride = stride; h->pg_has_values = values;
    return SOCCER_OK;
}

// a side's weights: finite, >= 0 and not all zero (NULL: every weight is 1.0 / n)
static int gradient_weights(soccer_handle* h, const char* what, const char* name, int n, const double* w, double* out) {
    bool any = false;
    for (int i = 0; i < n; ++i) {
        const double v = w ? w[i] : 1.0 / (double)n;
        if (!(v >= 0.0) || !(v <= DBL_MAX)) return fail(h, SOCCER_E_INVALID, "%s: %s[%d] is negative or not finite", what, name, i);
        any = any || v > 0.0;
        out[i] = v;
    }
    if (!any) return fail(h, SOCCER_E_INVALID, "%s: %s is all zero", what, name);
    return SOCCER_OK;
}

// soccer_cross_play's checks of everything but the policies
static int gradient_check(soccer_handle* h, const char* what, int32_t n_a, int32_t n_b, double theta, double discount_factor,
                          int32_t max_sweeps, int32_t pairs_per_pass) {
    if (int rc = minimax_check(h, what, discount_factor)) return rc;
    if (n_a < 1 || n_a > SOCCER_CROSS_MAX_POLICIES || n_b < 1 || n_b > SOCCER_CROSS_MAX_POLICIES)
        return fail(h, SOCCER_E_INVALID, "%s: the number of policies of each player must be 1 .. %d, not %d and %d", what,
                    SOCCER_CROSS_MAX_POLICIES, n_a, n_b);
    if (max_sweeps < 1) return fail(h, SOCCER_E_INVALID, "max_sweeps must be >= 1");
    if (!(theta >= 0.0)) return fail(h, SOCCER_E_INVALID, "theta must be >= 0");
    if (pairs_per_pass < 0 || pairs_per_pass % 64)
        return fail(h, SOCCER_E_INVALID, "%s: pairs_per_pass must be 0 (the library chooses) or a positive multiple of 64, not %d", what, pairs_per_pass);
    return SOCCER_OK;
}

struct GradientOut {                        // HOST pointers, any may be NULL
    double* payoff; double* grad_a; double* grad_b; double* reach_a; double* reach_b;
    double* q_a; double* q_b; double* V; double* occupancy; int32_t* iterations;
};

// behind every check: pa / pb are [n][nS][5] where `kind` says (the caller's, or a learner's on the device), w is w_a then w_b.
// With `keep` the gradients are formed whatever is asked for and stay in h->pg_grad (grad_a, then grad_b) for the caller.
static int gradient_solve(soccer_handle* h, const char* what, int n_a, const double* pa, int n_b, const double* pb, hipMemcpyKind kind,
                          double theta, double gamma, int32_t max_sweeps, int32_t pairs_per_pass, const std::vector<double>& w,
                          int normalize, bool keep, const GradientOut& out) {
    if (int rc = minimax_prepare(h)) return rc;
    if (int rc = build_occupancy_lists(h)) return rc;
    const int nS = h->mm.nS;
    const int total = n_a * n_b, total64 = (total + 63) / 64 * 64;
    // the library's choice: two V, two D and the ten action-value planes of a pass, 14 * nS * pairs * 8 bytes, stay at or under 1 GiB
    int per_pass = pairs_per_pass ? pairs_per_pass : std::max(64, (int)(((size_t)1 << 30) / ((size_t)112 * nS) / 64 * 64));
    per_pass = std::min(per_pass, total64);
    const bool grads = keep || out.grad_a || out.grad_b || out.reach_a || out.reach_b;
    const bool form_q = grads || out.q_a || out.q_b;
    if (int rc = gradient_buffers(h, n_a + n_b, per_pass, out.q_a || out.q_b || out.V || out.occupancy)) return rc;
    const int stride = h->pg_stride;                                    // (what an earlier, larger pass left: no result depends on it)
    const size_t rows = (size_t)nS * 5, cells = (size_t)nS * stride;
    double* d_x = h->pg_pol; double* d_y = h->pg_pol + (size_t)n_a * rows;
    double* d_xT = h->pg_polT; double* d_yT = h->pg_polT + (size_t)n_a * rows;
    double* d_grad_b = h->pg_grad + (size_t)n_a * rows; double* d_reach_b = h->pg_reach + (size_t)n_a * nS;
    double* d_Qa = h->pg_Q; double* d_Qb = h->pg_Q + cells * 5;
    if (int rc = response_upload(h, d_x, pa, n_a, kind)) return rc;
    if (int rc = response_upload(h, d_y, pb, n_b, kind)) return rc;
    occupancy_transposed(h, d_x, d_xT, n_a, d_y, d_yT, n_b);
    HIP_TRY(h, hipGetLastError());
    if (grads) {
        HIP_TRY(h, hipMemcpyAsync(h->pg_w, w.data(), (size_t)(n_a + n_b) * 8, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemsetAsync(h->pg_grad, 0, (size_t)(n_a + n_b) * rows * 8, h->stream));     // every sum starts from 0.0
        HIP_TRY(h, hipMemsetAsync(h->pg_reach, 0, (size_t)(n_a + n_b) * nS * 8, h->stream));
    }
    CrossIO cio{};
    cio.offset = h->mm.offset; cio.list = h->mm.list; cio.x = d_x; cio.y = d_y; cio.gamma = gamma; cio.theta = theta;
    cio.nS = nS; cio.n_b = n_b; cio.stride = stride; cio.last = total - 1;
    OccupancyIO oio{};
    oio.in_offset = h->oc_in_offset; oio.in_list = h->oc_in_list; oio.xT = d_xT; oio.yT = d_yT; oio.c = gamma; oio.theta = theta;
    oio.n_isd = h->rules.n_isd; oio.mu = 1.0 / (double)h->rules.n_isd;
    for (int i = 0; i < h->rules.n_isd; ++i) oio.isd[i] = (int32_t)h->rules.isd_obs[i];
    oio.nS = nS; oio.n_a = n_a; oio.n_b = n_b; oio.stride = stride; oio.last = total - 1;
    const PassBufs pass_V{{h->pg_V[0], h->pg_V[1]}, h->pg_words, h->pg_done[0], h->pg_open, stride};
    const PassBufs pass_D{{h->pg_D[0], h->pg_D[1]}, h->pg_words, h->pg_done[1], h->pg_open, stride};
    CrossFinishIO fio{};                                                // cross_finish_kernel's: the payoff
    fio.V[0] = h->pg_V[0]; fio.V[1] = h->pg_V[1]; fio.done_at = h->pg_done[0]; fio.payoff = h->pg_payoff; fio.iterations = h->pg_iter;
    fio.values = h->pg_values; fio.n_isd = h->rules.n_isd; fio.nS = nS; fio.stride = stride; fio.max_sweeps = max_sweeps;
    for (int i = 0; i < h->rules.n_isd; ++i) fio.isd[i] = (int32_t)h->rules.isd_obs[i];
    CrossFinishIO dio = fio;                                            // cross_values_kernel's: D is laid out like V
    dio.V[0] = h->pg_D[0]; dio.V[1] = h->pg_D[1]; dio.done_at = h->pg_done[1];
    CrossFinishIO qio = fio;                                            // ... and a plane of action values like a V of nS * 5 rows
    qio.nS = (int32_t)rows;
    ActionValuesIO aio{};
    aio.offset = h->mm.offset; aio.list = h->mm.list; aio.x = d_x; aio.y = d_y; aio.V[0] = h->pg_V[0]; aio.V[1] = h->pg_V[1];
    aio.done_at = h->pg_done[0]; aio.Qa = d_Qa; aio.Qb = d_Qb; aio.gamma = gamma; aio.nS = nS; aio.n_b = n_b; aio.stride = stride;
    aio.last = total - 1; aio.max_sweeps = max_sweeps;
    GradientReduceIO rio[2] = {};
    for (int side = 0; side < 2; ++side) {
        GradientReduceIO& r = rio[side];
        r.D[0] = h->pg_D[0]; r.D[1] = h->pg_D[1]; r.done_at = h->pg_done[1]; r.Q = side ? d_Qb : d_Qa;
        r.w = h->pg_w + (side ? 0 : n_a);                               // the other side's
        r.grad = side ? d_grad_b : h->pg_grad; r.reach = side ? d_reach_b : h->pg_reach;
        r.side = side; r.n_a = n_a; r.n_b = n_b; r.nS = nS; r.stride = stride; r.max_sweeps = max_sweeps;
    }
    std::vector<int32_t> done((size_t)2 * per_pass);
    int64_t open_total = 0;
    for (int first = 0; first < total; first += per_pass) {
        const int pairs = std::min(per_pass, total - first);
        const unsigned pair_blocks = (unsigned)((pairs + kCrossBlock - 1) / kCrossBlock), pair_waves = (unsigned)((pairs + 63) / 64);
        cio.first = first; cio.pairs = pairs; oio.first = first; oio.pairs = pairs;
        fio.pairs = pairs; dio.pairs = pairs; qio.pairs = pairs; aio.first = first; aio.pairs = pairs;
        // (the two counts of open pairs are not asked for: a pair is open if either solve is, which the stopping sweeps below tell)
        if (int rc = cross_solve_pass(h, cio, pass_V, max_sweeps, nullptr)) return rc;
        if (int rc = occupancy_solve_pass(h, oio, pass_D, max_sweeps, nullptr)) return rc;
        if (out.payoff) hipLaunchKernelGGL(cross_finish_kernel, dim3(pair_blocks), dim3(kCrossBlock), 0, h->stream, fio);
        if (form_q)
            hipLaunchKernelGGL(action_values_kernel, dim3((unsigned)((nS + kCrossWaves - 1) / kCrossWaves), pair_waves), dim3(kCrossBlock), 0, h->stream, aio);
        for (int side = 0; side < 2 && grads; ++side) {
            rio[side].first = first; rio[side].pairs = pairs;
            const size_t threads = (size_t)(side ? n_b : n_a) * nS;
            hipLaunchKernelGGL(gradient_reduce_kernel, dim3((unsigned)((threads + kCrossBlock - 1) / kCrossBlock)), dim3(kCrossBlock), 0, h->stream, rio[side]);
        }
        HIP_TRY(h, hipGetLastError());
        if (out.payoff) HIP_TRY(h, hipMemcpyAsync(out.payoff + first, h->pg_payoff, (size_t)pairs * 8, hipMemcpyDeviceToHost, h->stream));
        // V, D, q_a and q_b leave one after the other through the one transposed buffer (the stream keeps them in order)
        struct { double* dst; const CrossFinishIO* io; const double* plane; size_t width; } const leave[4] = {
            {out.V, &fio, nullptr, (size_t)nS}, {out.occupancy, &dio, nullptr, (size_t)nS}, {out.q_a, &qio, d_Qa, rows}, {out.q_b, &qio, d_Qb, rows}};
        for (const auto& l : leave) {
            if (!l.dst) continue;
            CrossFinishIO v = *l.io;
            if (l.plane) { v.V[0] = l.plane; v.V[1] = l.plane; }
            hipLaunchKernelGGL(cross_values_kernel, dim3(pair_waves, (unsigned)((l.width + 63) / 64)), dim3(kCrossBlock), 0, h->stream, v);
            HIP_TRY(h, hipGetLastError());
            HIP_TRY(h, hipMemcpyAsync(l.dst + (size_t)first * l.width, h->pg_values, (size_t)pairs * l.width * 8, hipMemcpyDeviceToHost, h->stream));
        }
        for (int c = 0; c < 2; ++c)
            HIP_TRY(h, hipMemcpyAsync(done.data() + (size_t)c * per_pass, h->pg_done[c], (size_t)pairs * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        for (int p = 0; p < pairs; ++p) {
            const int32_t kV = done[p], kD = done[(size_t)per_pass + p];
            if (!kV || !kD) ++open_total;
            if (out.iterations) {
                out.iterations[((size_t)first + p) * 2] = kV ? kV : max_sweeps;
                out.iterations[((size_t)first + p) * 2 + 1] = kD ? kD : max_sweeps;
            }
        }
    }
    if (grads) {
        if (normalize) {
            GradientNormalizeIO nio{};
            nio.grad = h->pg_grad; nio.reach = h->pg_reach; nio.rows = (int64_t)(n_a + n_b) * nS;     // both sides: grad_b follows grad_a
            hipLaunchKernelGGL(gradient_normalize_kernel, dim3((unsigned)((nio.rows + kCrossBlock - 1) / kCrossBlock)), dim3(kCrossBlock), 0, h->stream, nio);
            HIP_TRY(h, hipGetLastError());
        }
        if (out.grad_a) HIP_TRY(h, hipMemcpyAsync(out.grad_a, h->pg_grad, (size_t)n_a * rows * 8, hipMemcpyDeviceToHost, h->stream));
        if (out.grad_b) HIP_TRY(h, hipMemcpyAsync(out.grad_b, d_grad_b, (size_t)n_b * rows * 8, hipMemcpyDeviceToHost, h->stream));
        if (out.reach_a) HIP_TRY(h, hipMemcpyAsync(out.reach_a, h->pg_reach, (size_t)n_a * nS * 8, hipMemcpyDeviceToHost, h->stream));
        if (out.reach_b) HIP_TRY(h, hipMemcpyAsync(out.reach_b, d_reach_b, (size_t)n_b * nS * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if (open_total) return fail(h, SOCCER_E_STATE, "%s: %lld of %d pairs had not converged after max_sweeps = %d sweeps", what,
                                (long long)open_total, total, max_sweeps);
    return SOCCER_OK;
}

extern "C" int soccer_policy_gradient(soccer_handle* h, int32_t n_a, const double* pi_a, int32_t n_b, const double* pi_b, double theta,
                                      double discount_factor, int32_t max_sweeps, int32_t pairs_per_pass, const double* w_a,
                                      const double* w_b, int32_t normalize, double* payoff, double* grad_a, double* grad_b,
                                      double* reach_a, double* reach_b, double* q_a, double* q_b, double* V, double* occupancy,
                                      int32_t* iterations) {
    const char* what = "soccer_policy_gradient";
    if (int rc = gradient_check(h, what, n_a, n_b, theta, discount_factor, max_sweeps, pairs_per_pass)) return rc;
    if (int rc = response_rows(h, what, "pi_a", n_a, pi_a)) return rc;
    if (int rc = response_rows(h, what, "pi_b", n_b, pi_b)) return rc;
    std::vector<double> w((size_t)n_a + n_b);
    if (int rc = gradient_weights(h, what, "w_a", n_a, w_a, w.data())) return rc;
    if (int rc = gradient_weights(h, what, "w_b", n_b, w_b, w.data() + n_a)) return rc;
    const GradientOut out{payoff, grad_a, grad_b, reach_a, reach_b, q_a, q_b, V, occupancy, iterations};
    return gradient_solve(h, what, n_a, pi_a, n_b, pi_b, hipMemcpyHostToDevice, theta, discount_factor, max_sweeps, pairs_per_pass, w,
                          normalize, false, out);
}

// ------------------------------------------------------------------------------------------------
// gradient play: both sets of policies live on the device and take projected steps along soccer_policy_gradient's
// gradients of themselves.  A learner is owned by the handle (its own list: it shares nothing with the sampled learners of
// soccer_learners.hip) and freed with it.
struct soccer_gradient_play {
    OwnedBufs bufs{"the gradient-play learner"};
    soccer_gradient_play_config cfg{};
    double* pol = nullptr;                  // [n_a + n_b][nS][5] x, then y
    double* prev = nullptr;                 // [n_a + n_b][nS][5] the previous step's gradients
    int64_t steps = 0;
    std::vector<double> w;                  // w_a, then w_b
    std::vector<double> payoff;             // [n_a][n_b] the last completed step's, before its update
};

void gradient_players_release(soccer_handle* h) {
    for (soccer_gradient_play* g : h->gradient_players) delete g;
    h->gradient_players.clear();
}

// the caller's pointer is only compared with the handle's list, never read
static int gradient_play_check(soccer_handle* h, const soccer_gradient_play* g, const char* what) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "%s during graph capture", what);
    if (!g || std::find(h->gradient_players.begin(), h->gradient_players.end(), g) == h->gradient_players.end())
        return fail(h, SOCCER_E_INVALID, "%s: not a gradient-play learner of this handle", what);
    return SOCCER_OK;
}

extern "C" int soccer_gradient_play_create(soccer_handle* h, const soccer_gradient_play_config* cfg, soccer_gradient_play** out) {
    const char* what = "soccer_gradient_play_create";
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (!cfg || !out) return fail(h, SOCCER_E_INVALID, "%s: cfg and out are required", what);
    *out = nullptr;
    if (int rc = gradient_check(h, what, cfg->n_a, cfg->n_b, cfg->theta, cfg->discount_factor, cfg->max_sweeps, cfg->pairs_per_pass)) return rc;
    if (!(cfg->eta_a >= 0.0 && cfg->eta_a <= DBL_MAX) || !(cfg->eta_b >= 0.0 && cfg->eta_b <= DBL_MAX))
        return fail(h, SOCCER_E_INVALID, "%s: eta_a and eta_b must be finite and >= 0", what);
    if (!(cfg->optimism >= 0.0 && cfg->optimism <= 1.0)) return fail(h, SOCCER_E_INVALID, "%s: optimism must be in [0, 1]", what);
    if (cfg->pi_a) if (int rc = response_rows(h, what, "pi_a", cfg->n_a, cfg->pi_a)) return rc;
    if (cfg->pi_b) if (int rc = response_rows(h, what, "pi_b", cfg->n_b, cfg->pi_b)) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const int nS = h->rules.nS, n = cfg->n_a + cfg->n_b;
    const size_t rows = (size_t)nS * 5;
    soccer_gradient_play* g = new soccer_gradient_play();
    g->cfg = *cfg; g->cfg.pi_a = nullptr; g->cfg.pi_b = nullptr;
    g->w.resize((size_t)n); g->payoff.assign((size_t)cfg->n_a * cfg->n_b, 0.0);
    (void)gradient_weights(h, what, "w_a", cfg->n_a, nullptr, g->w.data());
    (void)gradient_weights(h, what, "w_b", cfg->n_b, nullptr, g->w.data() + cfg->n_a);
    int rc = g->bufs.alloc(h, (size_t)n * rows, &g->pol);
    if (!rc) rc = g->bufs.alloc(h, (size_t)n * rows, &g->prev);
    hipError_t e = hipSuccess;
    if (!rc) {
        const std::vector<double> uniform((size_t)std::max(cfg->n_a, cfg->n_b) * rows, 0.2);
        e = hipMemcpyAsync(g->pol, cfg->pi_a ? cfg->pi_a : uniform.data(), (size_t)cfg->n_a * rows * 8, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(g->pol + (size_t)cfg->n_a * rows, cfg->pi_b ? cfg->pi_b : uniform.data(), (size_t)cfg->n_b * rows * 8, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemsetAsync(g->prev, 0, (size_t)n * rows * 8, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) rc = fail(h, SOCCER_E_HIP, "%s failed: %s", what, hipGetErrorString(e));
    }
    if (rc) { delete g; return rc; }
    h->gradient_players.push_back(g);
    *out = g;
    return SOCCER_OK;
}

extern "C" int soccer_gradient_play_destroy(soccer_handle* h, soccer_gradient_play* g) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (!g) return SOCCER_OK;
    if (int rc = gradient_play_check(h, g, "soccer_gradient_play_destroy")) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));            // nothing is freed under a kernel that reads it
    h->gradient_players.erase(std::find(h->gradient_players.begin(), h->gradient_players.end(), g));
    delete g;
    return SOCCER_OK;
}

extern "C" int soccer_gradient_play_run(soccer_handle* h, soccer_gradient_play* g, int32_t n_steps, double* trace) {
    const char* what = "soccer_gradient_play_run";
    if (int rc = gradient_play_check(h, g, what)) return rc;
    if (n_steps < 0) return fail(h, SOCCER_E_INVALID, "%s: n_steps must be >= 0", what);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const soccer_gradient_play_config& c = g->cfg;
    const int nS = h->rules.nS;
    const size_t rows = (size_t)nS * 5, cells = (size_t)c.n_a * c.n_b;
    std::vector<double> payoff(cells);
    GradientOut out{};
    out.payoff = payoff.data();
    for (int32_t t = 0; t < n_steps; ++t) {
        // a step whose solves are still open is not applied: the state is that of the completed steps
        if (int rc = gradient_solve(h, what, c.n_a, g->pol, c.n_b, g->pol + (size_t)c.n_a * rows, hipMemcpyDeviceToDevice, c.theta,
                                    c.discount_factor, c.max_sweeps, c.pairs_per_pass, g->w, c.normalize, true, out)) return rc;
        GradientStepIO sio{};
        sio.pol = g->pol; sio.prev = g->prev; sio.grad = h->pg_grad; sio.eta_a = c.eta_a; sio.eta_b = c.eta_b; sio.optimism = c.optimism;
        sio.rows_a = (int64_t)c.n_a * nS; sio.rows = (int64_t)(c.n_a + c.n_b) * nS; sio.nS = nS; sio.first_step = g->steps == 0;
        hipLaunchKernelGGL(gradient_step_kernel, dim3((unsigned)((sio.rows + kCrossBlock - 1) / kCrossBlock)), dim3(kCrossBlock), 0, h->stream, sio);
        HIP_TRY(h, hipGetLastError());
        g->payoff = payoff;
        if (trace) std::memcpy(trace + (size_t)t * cells, payoff.data(), cells * 8);
        g->steps += 1;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SOCCER_OK;
}

extern "C" int soccer_gradient_play_read(soccer_handle* h, soccer_gradient_play* g, double* pi_a, double* pi_b, double* prev_a,
                                         double* prev_b, double* w_a, double* w_b, double* payoff, int64_t* steps) {
    if (int rc = gradient_play_check(h, g, "soccer_gradient_play_read")) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t rows = (size_t)h->rules.nS * 5, na = (size_t)g->cfg.n_a * rows, nb = (size_t)g->cfg.n_b * rows;
    if (pi_a) HIP_TRY(h, hipMemcpyAsync(pi_a, g->pol, na * 8, hipMemcpyDeviceToHost, h->stream));
    if (pi_b) HIP_TRY(h, hipMemcpyAsync(pi_b, g->pol + na, nb * 8, hipMemcpyDeviceToHost, h->stream));
    if (prev_a) HIP_TRY(h, hipMemcpyAsync(prev_a, g->prev, na * 8, hipMemcpyDeviceToHost, h->stream));
    if (prev_b) HIP_TRY(h, hipMemcpyAsync(prev_b, g->prev + na, nb * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (w_a) std::memcpy(w_a, g->w.data(), (size_t)g->cfg.n_a * 8);
    if (w_b) std::memcpy(w_b, g->w.data() + g->cfg.n_a, (size_t)g->cfg.n_b * 8);
    if (payoff) std::memcpy(payoff, g->payoff.data(), g->payoff.size() * 8);
    if (steps) *steps = g->steps;
    return SOCCER_OK;
}

extern "C" int soccer_gradient_play_load(soccer_handle* h, soccer_gradient_play* g, const double* pi_a, const double* pi_b,
                                         const double* prev_a, const double* prev_b, const double* payoff, const int64_t* steps) {
    const char* what = "soccer_gradient_play_load";
    if (int rc = gradient_play_check(h, g, what)) return rc;
    if (pi_a) if (int rc = response_rows(h, what, "pi_a", g->cfg.n_a, pi_a)) return rc;
    if (pi_b) if (int rc = response_rows(h, what, "pi_b", g->cfg.n_b, pi_b)) return rc;
    if (steps && *steps < 0) return fail(h, SOCCER_E_INVALID, "%s: steps must be >= 0", what);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t rows = (size_t)h->rules.nS * 5, na = (size_t)g->cfg.n_a * rows, nb = (size_t)g->cfg.n_b * rows;
    if (pi_a) HIP_TRY(h, hipMemcpyAsync(g->pol, pi_a, na * 8, hipMemcpyHostToDevice, h->stream));
    if (pi_b) HIP_TRY(h, hipMemcpyAsync(g->pol + na, pi_b, nb * 8, hipMemcpyHostToDevice, h->stream));
    if (prev_a) HIP_TRY(h, hipMemcpyAsync(g->prev, prev_a, na * 8, hipMemcpyHostToDevice, h->stream));
    if (prev_b) HIP_TRY(h, hipMemcpyAsync(g->prev + na, prev_b, nb * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (payoff) std::memcpy(g->payoff.data(), payoff, g->payoff.size() * 8);
    if (steps) g->steps = *steps;
    return SOCCER_OK;
}

extern "C" int soccer_gradient_play_set_weights(soccer_handle* h, soccer_gradient_play* g, const double* w_a, const double* w_b) {
    const char* what = "soccer_gradient_play_set_weights";
    if (int rc = gradient_play_check(h, g, what)) return rc;
    std::vector<double> w(g->w.size());
    if (int rc = gradient_weights(h, what, "w_a", g->cfg.n_a, w_a, w.data())) return rc;
    if (int rc = gradient_weights(h, what, "w_b", g->cfg.n_b, w_b, w.data() + g->cfg.n_a)) return rc;
    g->w = w;
    return SOCCER_OK;
}
