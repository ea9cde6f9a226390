// soccer_step.hip — batched_step / batched_step_ex: which single-step kernel a call gets, and its launch (see soccer_handle.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "soccer_dispatch.hpp"
#include "soccer_handle.hpp"
#include "soccer_step_kernels.hpp"

// the work list of step_kernel_swar<.., SLIPM = 3, ..>: one index per 4-lane group of the handle, then the count at an 8-byte aligned
// word at least 16 bytes behind them, then the tail kernel's two uint64 statistics (step_kernel: launch parts, groups walked)
static inline size_t worklist_count_word(const soccer_handle* h) { return ((size_t)(h->P.n >> 2) + 5) & ~(size_t)1; }
static inline uint32_t* worklist_count(const soccer_handle* h) { return h->d_worklist ? h->d_worklist + worklist_count_word(h) : nullptr; }
static bool ensure_worklist(soccer_handle* h) {
    if (h->d_worklist) return true;
    const size_t words = worklist_count_word(h) + 2 + 4;
    if (h->bufs.alloc(h, words, &h->d_worklist) != SOCCER_OK) { (void)hipGetLastError(); return false; }     // (no error: the per-lane kernel then)
    // (on the handle's own stream: a memset on the null stream is not ordered with a non-blocking stream's kernels)
    if (hipMemsetAsync(h->d_worklist, 0, words * sizeof(uint32_t), h->stream) != hipSuccess) {
        // without a cleared count the list must not be used: give it back, a later call tries again
        (void)hipGetLastError(); h->bufs.release(h->d_worklist); h->d_worklist = nullptr; return false;
    }
    return true;
}

// one launch_step as planned (soccer_launch_plan.hpp: plan_step_part)
static int launch_step(soccer_handle* h, const KernelParams& P, const StepIO& io, const StepLaunch& L) {
    const dim3 b(kBlock);
    const unsigned long long* tick_in = h->capturing ? P.tick_in : nullptr;
    const unsigned long long tick = (unsigned long long)(h->tick - 1);
    if (L.family == kStepSwar) {
        // the byte-parallel kernel (four lanes stay packed in their dwords, no rule-table reads)
        // every launch part covers a multiple of 4 lanes (h->swar_launch_lanes is one), so bit 0 of the lane count is free: it carries
        // the action-load policy into the kernel in a preloaded register (step_kernel_swar)
        const unsigned long long act_stream = L.act_stream ? 1ull : 0ull;
        // The kernel's byte offsets are 32-bit (soccer_kernels.hpp): a handle beyond kSwarLaunchLanes lanes is stepped by
        // several launches on the same tick, each handed its part of every stream; only the last one publishes the tick.
        for (unsigned long long c0 = P.first; c0 < P.first + P.n; c0 += h->swar_launch_lanes) {
            const unsigned long long cn = std::min<unsigned long long>(h->swar_launch_lanes, P.first + P.n - c0);
            const bool last = c0 + cn == P.first + P.n;
            const dim3 gh(static_cast<unsigned>(((cn >> 2) + kBlock - 1) / kBlock));
            SwarParams Q{h->swar_c, P.key0, P.key1, P.lane_offset + c0, last ? P.tick_out : nullptr, P.misuse,
                         off(io.obs, c0), off(io.reward, c0), off(io.terminated, c0), off(io.truncated, c0),
                         off(io.reward_a_f32, c0), off(io.reward_b_f32, c0), off(io.finished, c0), off(io.last_return, c0),
                         off(io.prob_code, c0), off(io.final_obs, c0),
                         P.step_stats ? P.hist : nullptr, P.hist_mask,
                         h->slip_c, reinterpret_cast<const swar::Quad*>(P.sub), h->d_slip_step_lut,
                         P.policy_a, P.policy_b, off(io.u_step, c0), off(io.u_reset, c0),
                         h->d_slip_f64, h->d_worklist, worklist_count(h)};
            const bool launched =
            with_value<0, 1, 2>(L.out, [&](auto ov) { return
            with_value<0, 1, 2, 3>(L.slipm, [&](auto sv) { return
            with_flag(L.policy, [&](auto pv) { return
            with_value<0, 1>(L.geo, [&](auto gv) { return
            with_flag(L.expl, [&](auto xv) { return
            with_flag(L.wide, [&](auto wv) {
                constexpr int OUT = decltype(ov)::value, SLIPM = decltype(sv)::value, GEO = decltype(gv)::value;
                constexpr bool POLICY = decltype(pv)::value, EXPL = decltype(xv)::value, WIDE = decltype(wv)::value;
                // caller-supplied uniforms come with SLIPM 0 or 3 only, and SLIPM 3 with nothing else; the wide layout with GEO 0 only
                constexpr bool compiled = (SLIPM == 3 ? EXPL : (!EXPL || SLIPM == 0)) && !(WIDE && GEO == 1);
                if constexpr (compiled)
                    hipLaunchKernelGGL((step_kernel_swar<OUT, SLIPM, POLICY, GEO, EXPL, WIDE ? kStateWide : kStatePacked>), gh, b, 0, h->stream,
                                       P.state + c0, P.state_stride, off(io.act_a, c0), off(io.act_b, c0), tick_in, cn | act_stream, tick, Q);
                return compiled;
            }); }); }); }); }); });
            if (!launched) return NOT_COMPILED(h, "step_kernel_swar");
            note_kernel(h);
            if (L.exact_tail) {
                // the groups of THIS part that were listed: the per-lane kernel, one workgroup, same tick (it publishes nothing)
                KernelParams R = P; R.first = c0; R.n = cn; R.tick_out = nullptr;
                StepIO jo = io; jo.worklist = h->d_worklist; jo.work_count = worklist_count(h);
                hipLaunchKernelGGL((step_kernel<true, true, true, true>), dim3(1), b, 0, h->stream, R, jo);
                note_kernel(h);
            }
        }
    } else if (L.family == kStepHot) {      // one 4-lane group per thread, as many workgroups as it takes
        const dim3 gh(static_cast<unsigned>(((P.n >> 2) + kBlock - 1) / kBlock));
        const bool launched =
        with_flag(L.slip, [&](auto slip) { return
        with_flag(L.int_only, [&](auto int_only) {
            constexpr bool compiled = decltype(slip)::value || !decltype(int_only)::value;      // (the integer-only decision is a slip decision)
            if constexpr (compiled)
                hipLaunchKernelGGL((step_kernel_hot<decltype(slip)::value, decltype(int_only)::value>), gh, b, 0, h->stream,
                                   P.state, P.state_stride, io.act_a, io.act_b, tick_in, P.n, tick, P, io);
            return compiled;
        }); });
        if (!launched) return NOT_COMPILED(h, "step_kernel_hot");
        note_kernel(h);
    } else {
        const dim3 g(grid_for(h, (P.n + 3) / 4));
        const bool launched =
        with_flag(L.slip, [&](auto slip) { return
        with_flag(L.explicit_u, [&](auto explicit_u) { return
        with_flag(L.vec, [&](auto vec) { return
        with_flag(L.shared, [&](auto shared) {
            constexpr bool EXPLICIT_U = decltype(explicit_u)::value, VEC = decltype(vec)::value, SHARED = decltype(shared)::value;
            // dword I/O on a shared phase or byte I/O; the draws of the kernel itself also with dword I/O off the phase
            constexpr bool compiled = VEC ? (SHARED || !EXPLICIT_U) : !SHARED;
            if constexpr (compiled)
                hipLaunchKernelGGL((step_kernel<decltype(slip)::value, EXPLICIT_U, VEC, SHARED>), g, b, 0, h->stream, P, io);
            return compiled;
        }); }); }); });
        if (!launched) return NOT_COMPILED(h, "step_kernel");
        note_kernel(h);
    }
    return SOCCER_OK;
}

// which pointers of a step are given and to what they are aligned
static StepCall step_call(const soccer_step_args* a) {
    StepCall c;
    // dword I/O needs every byte stream 4-aligned and the uint16 streams 8-aligned; else byte I/O
    c.dword_io = aligned(a->act_a, 4) && aligned(a->act_b, 4) && aligned(a->reward, 4) &&
                 aligned(a->terminated, 4) && aligned(a->truncated, 4) && aligned(a->prob_code, 4) &&
                 aligned(a->obs, 8) && aligned(a->final_obs, 8) && aligned(a->reward_a_f32, 16) && aligned(a->reward_b_f32, 16) &&
                 aligned(a->finished, 4);
    c.u_step = a->u_step; c.u_reset = a->u_reset; c.u_aligned16 = aligned(a->u_step, 16) && aligned(a->u_reset, 16);
    c.last_return = a->last_return; c.last_return_aligned4 = aligned(a->last_return, 4);
    c.full = a->prob_code || a->final_obs; c.gym = a->reward_a_f32 || a->reward_b_f32 || a->finished;
    return c;
}

// one step, one launch (two with a ragged tail); the arguments have been checked
static int launch_one_step(soccer_handle* h, const soccer_step_args* a) {
    HandleFacts f = handle_facts(h);
    const StepCall c = step_call(a);
    StepPlan S = plan_step(f, c);
    // the work list is allocated by the first call that will use it; where that fails the step takes the per-lane kernel
    if (S.main.exact_tail && !h->d_worklist && !ensure_worklist(h)) S = plan_step(f, c, true);
    KernelParams P = h->P;
    bind_tick(h, P, 1);
    StepIO io{a->act_a, a->act_b, a->u_step, a->u_reset, a->obs, a->reward, a->terminated, a->truncated,
              a->prob_code, a->final_obs, a->last_return, a->reward_a_f32, a->reward_b_f32, a->finished, nullptr, nullptr};
    const unsigned long long n = h->P.n, n4 = S.n4;
    if (n4) { P.first = 0; P.n = n4; if (int rc = launch_step(h, P, io, S.main)) return rc; }
    if (n4 < n) {               // ragged tail (or everything, when the buffers are not dword-aligned)
        KernelParams Q = P;
        Q.first = n4; Q.n = n - n4;
        if (n4) Q.tick_out = nullptr;   // same tick as the main launch, which publishes it
        if (int rc = launch_step(h, Q, io, S.rest)) return rc;
    }
    HIP_TRY(h, hipGetLastError());
    return SOCCER_OK;
}

// ---- captured steps: consecutive ones with evenly spaced rows are recorded as one rollout (include/soccer_hip.h) ----------
// the rollout a run of `len` steps from `f` on is
static soccer_rollout_args run_as_rollout(const soccer_step_args& f, int64_t len, int64_t act_stride, int64_t out_stride) {
    soccer_rollout_args r{};
    r.n_steps = (int32_t)len; r.sample_actions = 0;
    r.act_a = f.act_a; r.act_b = f.act_b; r.act_stride = act_stride;
    r.obs = f.obs; r.reward = f.reward; r.terminated = f.terminated; r.truncated = f.truncated; r.out_stride = out_stride;
    return r;
}

// may this step be part of a run at all: alone its plan is the byte-parallel kernel with OUT 0 (or, with step statistics, OUT 2 for
// the histogram only), and a run of such steps takes the byte-parallel rollout with its actions read from the two streams
static bool step_can_fuse(const soccer_handle* h, const soccer_step_args* a) {
    if (!h->graph_fuse || !h->own_stream) return false;
    const soccer_rollout_args r = run_as_rollout(*a, 1, (int64_t)h->P.n, (int64_t)h->P.n);
    return step_fusable(handle_facts(h), step_call(a), rollout_call(&r, nullptr, true));
}

// Over `len` steps no result stream may touch another stream of the run: a step's results must not be what a later step of
// the run reads or writes, because the fused launch keeps no order between lanes of different steps.  The two action streams
// are only read and may interleave ([T][2][n] blocks do).
static bool run_disjoint(const soccer_handle* h, const soccer_step_args& f, int64_t len, int64_t act_stride, int64_t out_stride) {
    struct Range { uintptr_t lo, hi; bool written; };
    const uint64_t n = h->P.n;
    Range r[6]; int m = 0;
    auto add = [&](const void* p, int64_t stride, size_t elem, bool written) {
        if (!p) return;
        const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
        r[m++] = Range{lo, lo + (uintptr_t)(((uint64_t)(len - 1) * (uint64_t)stride + n) * elem), written};
    };
    add(f.act_a, act_stride, 1, false); add(f.act_b, act_stride, 1, false);
    add(f.obs, out_stride, 2, true); add(f.reward, out_stride, 1, true);
    add(f.terminated, out_stride, 1, true); add(f.truncated, out_stride, 1, true);
    for (int i = 0; i < m; ++i)
        for (int j = i + 1; j < m; ++j)
            if ((r[i].written || r[j].written) && r[i].lo < r[j].hi && r[j].lo < r[i].hi) return false;
    return true;
}

// does step `a` continue the pending run?  The second step of a run fixes the two strides.
static bool run_extends(soccer_handle* h, const soccer_step_args* a) {
    PendingRun& R = h->run;
    const soccer_step_args& f = R.first;
    if (R.len < 1 || R.len >= (int64_t)1 << 30) return false;
    if (!a->obs != !f.obs || !a->reward != !f.reward || !a->terminated != !f.terminated || !a->truncated != !f.truncated) return false;
    const int64_t n = (int64_t)h->P.n;
    // elements from the run's first row to this step's (addresses as integers: the rows need not lie in one allocation)
    auto rows = [](const void* p, const void* q, int64_t elem) { return (int64_t)(reinterpret_cast<intptr_t>(p) - reinterpret_cast<intptr_t>(q)) / elem; };
    const int64_t da = rows(a->act_a, f.act_a, 1);
    int64_t d_out = 0;
    bool have = false, same = rows(a->act_b, f.act_b, 1) == da;
    auto out = [&](const void* p, const void* q, int64_t elem) {
        if (!q) return;
        const int64_t d = rows(p, q, elem);
        if (!have) { d_out = d; have = true; } else if (d != d_out) same = false;
    };
    out(a->obs, f.obs, 2); out(a->reward, f.reward, 1); out(a->terminated, f.terminated, 1); out(a->truncated, f.truncated, 1);
    if (!same) return false;
    int64_t as = R.act_stride, os = R.out_stride;
    if (R.len == 1) {
        as = da; os = have ? d_out : n;     // (no result stream: nothing is spaced by the output stride)
        if (as < n || as % 4 != 0 || os < n || os % 4 != 0) return false;
    } else if (da != R.len * as || (have && d_out != R.len * os)) return false;
    if (!run_disjoint(h, f, R.len + 1, as, os)) return false;
    R.act_stride = as; R.out_stride = os;
    return true;
}

int flush_run(soccer_handle* h) {
    const PendingRun R = h->run;
    h->run = PendingRun{};
    if (R.len < 1) return SOCCER_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));     // (the caller may be soccer_graph_end or a call that has not set it yet)
    if (R.len == 1) return launch_one_step(h, &R.first);
    const soccer_rollout_args r = run_as_rollout(R.first, R.len, R.act_stride, R.out_stride);
    // a step counts finished episodes only with SOCCER_F_STEP_STATS: without it the run takes the kernel's shape that does not
    // count (no histogram at all); soccer_rollout_shape keeps describing the caller's own last rollout
    const soccer_rollout_shape_info keep = h->last_rollout;
    const int rc = rollout_enqueue(h, &r, nullptr, h->P.step_stats ? h->d_hist : nullptr);
    h->last_rollout = keep;
    if (rc == SOCCER_OK) { h->capture_steps_fused += R.len; h->capture_fused_launches += 1; }
    return rc;
}

extern "C" int batched_step_ex(soccer_handle* h, const soccer_step_args* a) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (!a || (!a->act_a && !h->P.policy_a) || (!a->act_b && !h->P.policy_b))
        return fail(h, SOCCER_E_INVALID, "batched_step: an action stream is required for every player without a fixed policy");
    if (!aligned(a->u_step, 8) || !aligned(a->u_reset, 8) || !aligned(a->obs, 2) || !aligned(a->final_obs, 2) ||
        !aligned(a->reward_a_f32, 4) || !aligned(a->reward_b_f32, 4))
        return fail(h, SOCCER_E_INVALID, "batched_step: u_* must be 8-byte, reward_*_f32 4-byte and obs/final_obs 2-byte aligned");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (h->capturing) {
        // nothing is launched yet: the step joins the pending run, or ends it and starts the next one
        const bool can = step_can_fuse(h, a);
        if (can && h->run.len && run_extends(h, a)) { h->run.len += 1; return SOCCER_OK; }
        if (int rc = flush_pending(h)) return rc;
        if (can) { h->run.first = *a; h->run.len = 1; return SOCCER_OK; }
    }
    return launch_one_step(h, a);
}

extern "C" int batched_step(soccer_handle* h, const int8_t* act_a, const int8_t* act_b, uint16_t* obs,
                            int8_t* reward, uint8_t* terminated, uint8_t* truncated, uint8_t* prob_code) {
    soccer_step_args a{};
    a.act_a = act_a; a.act_b = act_b; a.obs = obs; a.reward = reward;
    a.terminated = terminated; a.truncated = truncated; a.prob_code = prob_code;
    return batched_step_ex(h, &a);
}

// what the work list's tail launches have walked so far (the two statistics behind the count, see worklist_count_word)
extern "C" int soccer_exact_walk_stats(const soccer_handle* h, uint64_t* parts, uint64_t* groups) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    soccer_handle* hm = const_cast<soccer_handle*>(h);                  // (the error text only)
    if (h->capturing) return fail(hm, SOCCER_E_STATE, "soccer_exact_walk_stats during graph capture");
    unsigned long long st[2] = {0ull, 0ull};
    if (h->d_worklist) {
        HIP_TRY(hm, hipSetDevice(h->cfg.device));
        HIP_TRY(hm, hipStreamSynchronize(h->stream));
        HIP_TRY(hm, hipMemcpy(st, worklist_count(h) + 2, sizeof st, hipMemcpyDeviceToHost));
    }
    if (parts) *parts = st[0];
    if (groups) *groups = st[1];
    return SOCCER_OK;
}
