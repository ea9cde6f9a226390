// soccer_planners.hip — the transition table, the single-agent planners, minimax value iteration, best responses to mixed policies, and the matrix-game solver (see soccer_handle.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
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

int minimax_check(soccer_handle* h, const char* what, double gamma) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "%s during graph capture", what);
    if (h->P.policy_a != nullptr || h->P.policy_b != nullptr)
        return fail(h, SOCCER_E_INVALID, "%s needs a two-player handle: neither side may have a fixed policy (soccer_set_policy)", what);
    if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(h, SOCCER_E_INVALID, "discount_factor must be in [0, 1]");
    return SOCCER_OK;
}

// after every argument is checked: the device and the cached lists
int minimax_prepare(soccer_handle* h) {
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
int response_rows(soccer_handle* h, const char* what, const char* name, int n, const double* pol) {
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
int response_upload(soccer_handle* h, double* dst, const double* pol, int n, hipMemcpyKind kind) {
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
