// soccer_step.hip — batched_step / batched_step_ex: which single-step kernel a call gets, and its launch (see soccer_handle.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>

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

template <bool EXPLICIT_U, bool VEC, bool SHARED>
static void launch_step3(soccer_handle* h, const KernelParams& P, const StepIO& io) {
    const int grid = grid_for(h, (P.n + 3) / 4);
    const dim3 g(grid), b(kBlock);
    if (h->slip) hipLaunchKernelGGL((step_kernel<true, EXPLICIT_U, VEC, SHARED>), g, b, 0, h->stream, P, io);
    else hipLaunchKernelGGL((step_kernel<false, EXPLICIT_U, VEC, SHARED>), g, b, 0, h->stream, P, io);
    note_kernel(h);
}
static void launch_step(soccer_handle* h, const KernelParams& P, const StepIO& io, bool explicit_u, bool vec) {
    const bool shared = ((P.lane_offset + P.first) & 3ull) == 0ull;
    const bool policy_only = explicit_u && !io.u_step && !io.u_reset;       // fixed-policy handle, Philox draws
    const bool swar_fit = vec && shared && h->swar_ok && (!h->slip || h->slip_swar_ok) && aligned(io.last_return, 4);
    // caller-supplied uniforms at slip_prob == 0: floor(4u) is the reference's decision for any double (step_kernel_swar, EXPL)
    const bool expl = explicit_u && !policy_only && !h->slip && aligned(io.u_step, 16) && aligned(io.u_reset, 16);
    // ... and at slip_prob > 0 the float64 decision against the nominal thresholds (SLIPM = 3); the groups it cannot decide safely go
    // to the per-lane kernel's exact walk through a work list (one extra small launch per call)
    const bool expl_slip = explicit_u && !policy_only && h->slip && io.u_step && aligned(io.u_step, 16) && aligned(io.u_reset, 16) &&
                           vec && shared && h->swar_ok && aligned(io.last_return, 4) && (P.n >> 2) < 0xffffffffull &&
                           (h->d_worklist || (!h->capturing && ensure_worklist(h)));      // (no allocation inside a capture: the per-lane kernel then)
    if (((policy_only || !explicit_u || expl) && swar_fit) || expl_slip) {
        // the byte-parallel kernel (four lanes stay packed in their dwords, no rule-table reads)
        // which outputs the launch needs decides the instantiation: 0 the four result streams, 1 + the gym floats /
        // finished / last_return, 2 + final_obs / prob_code / episode histogram
        const int out = (io.prob_code || io.final_obs || P.step_stats) ? 2
                      : (io.reward_a_f32 || io.reward_b_f32 || io.finished || io.last_return) ? 1 : 0;
        const dim3 b(kBlock);
        // every launch part covers a multiple of 4 lanes (h->swar_launch_lanes is one), so bit 0 of the lane count is free: it carries
        // the action-load policy into the kernel in a preloaded register (step_kernel_swar)
        const unsigned long long act_stream = (h->cfg.flags & SOCCER_F_STREAM_ACTIONS) ? 1ull : 0ull;
#define SWAR_ARGS P.state + c0, P.state_stride, off(io.act_a, c0), off(io.act_b, c0), (h->capturing ? P.tick_in : nullptr), cn | act_stream, (unsigned long long)(h->tick - 1), Q
        // six-stream handles that fit the byte arithmetic are host-mapped facade handles, tall pitches and SOCCER_STATE_LAYOUT=wide:
        // nobody times them, so they take the arithmetic geometry (GEO = 0, right for every pitch) instead of mirroring every shape
#define SWAR_GO(OV, SV, PV, XV) do { if (P.state_layout == kStateWide) hipLaunchKernelGGL((step_kernel_swar<OV, SV, PV, 0, XV, kStateWide>), gh, b, 0, h->stream, SWAR_ARGS); \
                                     else if (h->swar_c.small) hipLaunchKernelGGL((step_kernel_swar<OV, SV, PV, 1, XV, kStatePacked>), gh, b, 0, h->stream, SWAR_ARGS); \
                                     else hipLaunchKernelGGL((step_kernel_swar<OV, SV, PV, 0, XV, kStatePacked>), gh, b, 0, h->stream, SWAR_ARGS); } while (0)
#define SWAR_SLIP(OV, PV) do { if (expl_slip) SWAR_GO(OV, 3, PV, true); else if (expl) SWAR_GO(OV, 0, PV, true); else if (!h->slip) SWAR_GO(OV, 0, PV, false); \
                               else if (h->d_slip_step_lut) SWAR_GO(OV, 2, PV, false); else SWAR_GO(OV, 1, PV, false); } while (0)
#define SWAR_OUT(PV) do { if (out == 2) SWAR_SLIP(2, PV); else if (out == 1) SWAR_SLIP(1, PV); else SWAR_SLIP(0, PV); } while (0)
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
            if (P.policy_a || P.policy_b) SWAR_OUT(true); else SWAR_OUT(false);
            note_kernel(h);
            if (expl_slip) {
                // the groups of THIS part that were listed: the per-lane kernel, one workgroup, same tick (it publishes nothing)
                KernelParams R = P; R.first = c0; R.n = cn; R.tick_out = nullptr;
                StepIO jo = io; jo.worklist = h->d_worklist; jo.work_count = worklist_count(h);
                hipLaunchKernelGGL((step_kernel<true, true, true, true>), dim3(1), dim3(kBlock), 0, h->stream, R, jo);
                note_kernel(h);
            }
        }
#undef SWAR_OUT
#undef SWAR_SLIP
#undef SWAR_GO
#undef SWAR_ARGS
    } else if (explicit_u) {    // caller-supplied uniforms (facade, tests) and fixed-policy handles beyond the byte arithmetic: generic kernel
        if (vec && shared) launch_step3<true, true, true>(h, P, io); else launch_step3<true, false, false>(h, P, io);
    } else if (vec && shared) {
        // the per-lane kernels (slip handles, pitches beyond the byte arithmetic): step_kernel_hot has no code for
        // prob_code / final_obs / last_return / the gym outputs / step stats, step_kernel writes them
        const bool lean = !io.prob_code && !io.final_obs && !io.last_return && !io.reward_a_f32 && !io.reward_b_f32 && !io.finished && !P.step_stats;
        const int grid = grid_for(h, (P.n + 3) / 4);
        const dim3 g(grid), b(kBlock);
        if (lean) {                 // one 4-lane group per thread, as many workgroups as it takes
            const unsigned long long blocks = ((P.n >> 2) + kBlock - 1) / kBlock;
            const dim3 gh(static_cast<unsigned>(blocks));
#define HOT_ARGS P.state, P.state_stride, io.act_a, io.act_b, (h->capturing ? P.tick_in : nullptr), P.n, (unsigned long long)(h->tick - 1), P, io
            if (h->slip && P.slip_int == 1u) hipLaunchKernelGGL((step_kernel_hot<true, true>), gh, b, 0, h->stream, HOT_ARGS);
            else if (h->slip) hipLaunchKernelGGL(step_kernel_hot<true>, gh, b, 0, h->stream, HOT_ARGS);
            else hipLaunchKernelGGL(step_kernel_hot<false>, gh, b, 0, h->stream, HOT_ARGS);
            note_kernel(h);
#undef HOT_ARGS
        } else launch_step3<false, true, true>(h, P, io);
    }
    else if (vec) launch_step3<false, true, false>(h, P, io);
    else launch_step3<false, false, false>(h, P, io);
}

// one step, one launch (two with a ragged tail); the arguments have been checked
static int launch_one_step(soccer_handle* h, const soccer_step_args* a) {
    // dword I/O needs every byte stream 4-aligned and the uint16 streams 8-aligned; else byte I/O
    const bool vec = h->E != 1 && aligned(a->act_a, 4) && aligned(a->act_b, 4) && aligned(a->reward, 4) &&
                     aligned(a->terminated, 4) && aligned(a->truncated, 4) && aligned(a->prob_code, 4) &&
                     aligned(a->obs, 8) && aligned(a->final_obs, 8) && aligned(a->reward_a_f32, 16) && aligned(a->reward_b_f32, 16) &&
                     aligned(a->finished, 4);
    const bool explicit_u = a->u_step || a->u_reset || h->P.policy_a || h->P.policy_b;   // generic kernel
    KernelParams P = h->P;
    bind_tick(h, P, 1);
    StepIO io{a->act_a, a->act_b, a->u_step, a->u_reset, a->obs, a->reward, a->terminated, a->truncated,
              a->prob_code, a->final_obs, a->last_return, a->reward_a_f32, a->reward_b_f32, a->finished, nullptr, nullptr};
    const unsigned long long n = h->P.n, n4 = vec ? (n & ~3ull) : 0ull;
    if (n4) { P.first = 0; P.n = n4; launch_step(h, P, io, explicit_u, true); }
    if (n4 < n) {               // ragged tail (or everything, when the buffers are not dword-aligned)
        KernelParams Q = P;
        Q.first = n4; Q.n = n - n4;
        if (n4) Q.tick_out = nullptr;   // same tick as the main launch, which publishes it
        launch_step(h, Q, io, explicit_u, false);
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

// may this step be part of a run at all: alone it takes step_kernel_swar<0, ..> (or, with step statistics, <2, ..> for the
// histogram only), and a run of such steps takes the byte-parallel rollout with its actions read from the two streams
static bool step_can_fuse(const soccer_handle* h, const soccer_step_args* a) {
    if (!h->graph_fuse || !h->own_stream || h->P.policy_a || h->P.policy_b || h->E == 1 || (h->P.n & 3ull)) return false;
    if (a->u_step || a->u_reset || a->reward_a_f32 || a->reward_b_f32 || a->finished || a->last_return || a->prob_code || a->final_obs) return false;
    const soccer_rollout_args r = run_as_rollout(*a, 1, (int64_t)h->P.n, (int64_t)h->P.n);
    return rollout_takes_swar(h, &r, nullptr);
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
