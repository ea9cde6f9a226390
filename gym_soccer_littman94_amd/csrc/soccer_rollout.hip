// soccer_rollout.hip — batched_rollout / batched_rollout_ex: T fused steps per launch (see soccer_handle.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "soccer_dispatch.hpp"
#include "soccer_handle.hpp"
#include "soccer_rollout_kernels.hpp"
#include "soccer_slip.hpp"

static_assert(kSlipLutWords == kSlipLdsWords, "table layout shared with the kernels");      // soccer_create builds the image
static_assert(kPlanBlock == kBlock && kPlanSlipLutBytes == kSlipLutWords * sizeof(uint32_t), "the plan sizes LDS as the kernels use it");

hipError_t rollout_raise_smem_limit(const soccer_handle* h, size_t bytes) {
    hipError_t se = hipSuccess;
    for (int e : {1, 4, 8})
        for (bool d : {false, true})
            if (se == hipSuccess)
                se = with_value<1, 4, 8>(e, [&](auto ev) { return with_flag(d, [&](auto dyn) { return with_shape(h, [&](auto slip, auto lds) {
                    return hipFuncSetAttribute(reinterpret_cast<const void*>(&rollout_kernel<decltype(ev)::value, decltype(slip)::value, decltype(lds)::value, decltype(dyn)::value>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
                }); }); });
    return se;
}

// the per-lane kernel: rollout_kernel<E, slip, lut_lds, dyn> of the plan (the tail of a byte-parallel rollout: E = 1)
static int launch_rollout(soccer_handle* h, const RolloutPlan& R, int E, const KernelParams& P, const RolloutIO& io) {
    const dim3 g(grid_for(h, (P.n + E - 1) / E)), b(kBlock);
    const bool launched =
    with_value<8, 4, 1>(E, [&](auto ev) { return
    with_flag(R.slip, [&](auto slip) { return
    with_flag(R.lut_lds, [&](auto lds) { return
    with_flag(R.dyn, [&](auto dv) {
        hipLaunchKernelGGL((rollout_kernel<decltype(ev)::value, decltype(slip)::value, decltype(lds)::value, decltype(dv)::value>), g, b, h->smem_bytes, h->stream, P, io);
        return true;
    }); }); }); });
    if (!launched) return NOT_COMPILED(h, "rollout_kernel");
    note_kernel(h);
    return SOCCER_OK;
}

// the byte-parallel kernel: rollout_swar_kernel<dm, sm, geo, full, stats>, its LDS limit raised where the launch needs more than 48 KB
static int launch_rollout_swar(soccer_handle* h, const RolloutPlan& R, dim3 g, const RolloutSwar& RS, const RolloutIO& io) {
    hipError_t se = hipSuccess;
    const bool launched =
    with_value<0, 1, 2, 3, 4, 5>(R.dm, [&](auto dv) { return
    with_value<0, 1, 2>(R.sm, [&](auto sv) { return
    with_value<0, 1>(R.geo, [&](auto gv) { return
    with_flag(R.full, [&](auto fv) { return
    with_flag(R.stats, [&](auto tv) {
        constexpr int DM = decltype(dv)::value, SM = decltype(sv)::value, GEO = decltype(gv)::value;
        constexpr bool FULL = decltype(fv)::value, STATS = decltype(tv)::value;
        // the shape without statistics exists for streamed actions and the plain result streams only
        constexpr bool compiled = STATS || kUnreadShape<DM, FULL>;
        if constexpr (compiled) {
            if (R.smem > 48 * 1024)
                se = hipFuncSetAttribute(reinterpret_cast<const void*>(&rollout_swar_kernel<DM, SM, GEO, FULL, STATS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)R.smem);
            if (se == hipSuccess) hipLaunchKernelGGL((rollout_swar_kernel<DM, SM, GEO, FULL, STATS>), g, dim3(kBlock), R.smem, h->stream, RS, io);
        }
        return compiled;
    }); }); }); }); });
    if (!launched) return NOT_COMPILED(h, "rollout_swar_kernel");
    if (se != hipSuccess)
        return fail(h, se == hipErrorOutOfMemory ? SOCCER_E_NOMEM : SOCCER_E_HIP, "hipFuncSetAttribute(rollout_swar_kernel, %zu bytes of dynamic LDS) failed: %s",
                    R.smem, hipGetErrorString(se));
    note_kernel(h);
    return SOCCER_OK;
}

extern "C" int batched_rollout(soccer_handle* h, const soccer_rollout_args* a) { return batched_rollout_ex(h, a, nullptr); }

extern "C" int soccer_rollout_shape(const soccer_handle* h, soccer_rollout_shape_info* out) {
    if (!h || !out) return SOCCER_E_INVALID;
    *out = h->last_rollout;
    out->lds_limit = h->lds_limit;
    return SOCCER_OK;
}

extern "C" int batched_rollout_ex(soccer_handle* h, const soccer_rollout_args* a, const soccer_rollout_extra* x) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (int rc = flush_pending(h)) return rc;       // captured steps before this call come first
    if (!a || a->n_steps < 1) return fail(h, SOCCER_E_INVALID, "batched_rollout: n_steps must be >= 1");
    if (!a->sample_actions && ((!a->act_a && !h->P.policy_a) || (!a->act_b && !h->P.policy_b)))
        return fail(h, SOCCER_E_INVALID, "batched_rollout: an action stream is required for every player without a fixed policy (or sample_actions)");
    if (!a->sample_actions && a->act_stride < (int64_t)h->P.n)
        return fail(h, SOCCER_E_INVALID, "batched_rollout: act_stride must be >= n_lanes");
    uint16_t* x_fin = x ? x->final_obs : nullptr; uint8_t* x_code = x ? x->prob_code : nullptr;
    const bool any_out = a->obs || a->reward || a->terminated || a->truncated || x_fin || x_code;
    if (!aligned(x_fin, 2)) return fail(h, SOCCER_E_INVALID, "batched_rollout_ex: final_obs must be 2-byte aligned");
    if (any_out && a->out_stride < (int64_t)h->P.n)
        return fail(h, SOCCER_E_INVALID, "batched_rollout: out_stride must be >= n_lanes");
    if (!aligned(a->obs, 2) || !aligned(a->return_sum, 4) || !aligned(a->episode_count, 4) ||
        !aligned(a->mix_a, 8) || !aligned(a->mix_b, 8))
        return fail(h, SOCCER_E_INVALID, "batched_rollout: misaligned obs/return_sum/episode_count/mix_*");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return rollout_enqueue(h, a, x, h->P.hist);
}

// hist == nullptr: nobody reads this rollout's episode statistics (flush_run on a handle without step statistics) — the
// byte-parallel kernel then takes its shape that does not count; only a run that step_can_fuse admits may ask for it
int rollout_enqueue(soccer_handle* h, const soccer_rollout_args* a, const soccer_rollout_extra* x, unsigned long long* hist) {
    uint16_t* x_fin = x ? x->final_obs : nullptr; uint8_t* x_code = x ? x->prob_code : nullptr;
    const HandleFacts f = handle_facts(h);
    const RolloutPlan R = plan_rollout(f, rollout_call(a, x, hist != nullptr));
    if (R.refused) return fail(h, SOCCER_E_STATE, "rollout without statistics: not the shape of a fused run of captured steps");
    // one launch covers at most kChunk steps (per-thread episode counters are 16 bit wide); the tick
    // sequence of consecutive launches is contiguous, so chunking does not change any result
    constexpr int kChunk = 4096;
    for (int s0 = 0; s0 < a->n_steps; s0 += kChunk) {
        const int ns = a->n_steps - s0 < kChunk ? a->n_steps - s0 : kChunk;
        KernelParams P = h->P;
        P.hist = hist;
        bind_tick(h, P, (uint64_t)ns);
        const long long ao = (long long)s0 * a->act_stride, oo = (long long)s0 * a->out_stride;
        const RolloutIO io0{ns, a->sample_actions, a->mix_a, a->mix_b, a->act_a ? a->act_a + ao : nullptr, a->act_b ? a->act_b + ao : nullptr,
                            (long long)a->act_stride, a->obs ? a->obs + oo : nullptr, a->reward ? a->reward + oo : nullptr,
                            a->terminated ? a->terminated + oo : nullptr, a->truncated ? a->truncated + oo : nullptr,
                            (long long)a->out_stride, a->return_sum, a->episode_count, x_fin ? x_fin + oo : nullptr, x_code ? x_code + oo : nullptr};
        int parts = 0;
        if (R.swar) {
            const RolloutSwar RS0{P.state, P.state_stride, P.state_layout, P.first, R.n4, P.lane_offset, P.tick_in, P.tick_out, P.hist, P.misuse,
                                  P.policy_a, P.policy_b, P.key0, P.key1,
                                  h->swar_c, h->slip_c, reinterpret_cast<const swar::Quad*>(P.sub), P.hist_mask, h->rules.nS,
                                  R.lds_tables ? 1 : 0, R.act_off, R.tab_off, h->d_slip_lut};
            // The kernel's byte offsets are 32-bit: a handle beyond kSwarLaunchLanes lanes is rolled out part by part (lanes never
            // interact), every part over the same ticks, each handed its piece of every stream; the last one publishes the tick.
            for (unsigned long long c0 = 0; c0 < R.n4; c0 += h->swar_launch_lanes, ++parts) {
                const unsigned long long cn = std::min<unsigned long long>(h->swar_launch_lanes, R.n4 - c0);
                RolloutSwar RS = RS0; RolloutIO io = io0;
                RS.state = RS0.state + P.first + c0; RS.first = 0ull; RS.n = cn; RS.lane_offset = RS0.lane_offset + P.first + c0;
                if (c0 + cn < R.n4) RS.tick_out = nullptr;
                const unsigned long long lane0 = P.first + c0;
                io.act_a = off(io0.act_a, lane0); io.act_b = off(io0.act_b, lane0); io.obs = off(io0.obs, lane0); io.reward = off(io0.reward, lane0);
                io.terminated = off(io0.terminated, lane0); io.truncated = off(io0.truncated, lane0);
                io.return_sum = off(io0.return_sum, lane0); io.episode_count = off(io0.episode_count, lane0);
                io.final_obs = off(io0.final_obs, lane0); io.prob_code = off(io0.prob_code, lane0);
                uint64_t blocks = ((cn >> 2) + kBlock - 1) / kBlock;
                if (blocks > (uint64_t)h->grid_cap) blocks = h->grid_cap;
                if (int rc = launch_rollout_swar(h, R, dim3((unsigned)blocks), RS, io)) return rc;
            }
            if (R.tail) {
                KernelParams Q = h->P;
                Q.hist = hist;
                Q.tick_in = P.tick_in; Q.tick_out = nullptr;      // the main launch publishes the tick
                Q.first = R.n4; Q.n = f.n - R.n4;
                if (int rc = launch_rollout(h, R, 1, Q, io0)) return rc;    // (the per-lane kernel indexes by absolute lane)
            }
        } else if (int rc = launch_rollout(h, R, R.E, P, io0)) return rc;
        h->last_rollout = rollout_shape_of(f, R, parts, (a->n_steps + kChunk - 1) / kChunk);
        HIP_TRY(h, hipGetLastError());
    }
    return SOCCER_OK;
}
