// soccer_rollout.hip — batched_rollout / batched_rollout_ex: T fused steps per launch (see soccer_handle.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "soccer_handle.hpp"
#include "soccer_rollout_kernels.hpp"
#include "soccer_slip.hpp"

static_assert(kSlipLutWords == kSlipLdsWords, "table layout shared with the kernels");      // soccer_create builds the image

template <int E, bool SLIP, bool LUT_LDS>
static hipError_t raise_smem_limit(size_t bytes) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&rollout_kernel<E, SLIP, LUT_LDS, false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&rollout_kernel<E, SLIP, LUT_LDS, true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

hipError_t rollout_raise_smem_limit(const soccer_handle* h, size_t bytes) {
    hipError_t se = hipSuccess;
#define RAISE(EV) if (se == hipSuccess) { se = h->slip ? (h->lut_lds ? raise_smem_limit<EV, true, true>(bytes) : raise_smem_limit<EV, true, false>(bytes)) \
                                                       : (h->lut_lds ? raise_smem_limit<EV, false, true>(bytes) : raise_smem_limit<EV, false, false>(bytes)); }
    RAISE(1) RAISE(4) RAISE(8)
#undef RAISE
    return se;
}

template <int E, bool DYN>
static void launch_rollout2(soccer_handle* h, const KernelParams& P, const RolloutIO& io) {
    const int grid = grid_for(h, (P.n + E - 1) / E);
    const dim3 g(grid), b(kBlock);
    if (h->slip) {
        if (h->lut_lds) hipLaunchKernelGGL((rollout_kernel<E, true, true, DYN>), g, b, h->smem_bytes, h->stream, P, io);
        else hipLaunchKernelGGL((rollout_kernel<E, true, false, DYN>), g, b, h->smem_bytes, h->stream, P, io);
    } else {
        if (h->lut_lds) hipLaunchKernelGGL((rollout_kernel<E, false, true, DYN>), g, b, h->smem_bytes, h->stream, P, io);
        else hipLaunchKernelGGL((rollout_kernel<E, false, false, DYN>), g, b, h->smem_bytes, h->stream, P, io);
    }
    note_kernel(h);
}
template <int E>
static void launch_rollout(soccer_handle* h, const KernelParams& P, const RolloutIO& io) {
    // DYN: some action is produced in the kernel (sampling, mixed policy, fixed policy)
    const bool dyn = io.sample_actions || P.policy_a || P.policy_b;
    if (dyn) launch_rollout2<E, true>(h, P, io); else launch_rollout2<E, false>(h, P, io);
}

extern "C" int batched_rollout(soccer_handle* h, const soccer_rollout_args* a) { return batched_rollout_ex(h, a, nullptr); }

extern "C" int soccer_rollout_shape(const soccer_handle* h, soccer_rollout_shape_info* out) {
    if (!h || !out) return SOCCER_E_INVALID;
    *out = h->last_rollout;
    out->lds_limit = h->lds_limit;
    return SOCCER_OK;
}

// dword (e = 4) or wider I/O needs every stream aligned to e of its elements and both strides multiples of e
static bool rollout_vec_ok(const soccer_rollout_args* a, const soccer_rollout_extra* x, int e) {
    const uint16_t* x_fin = x ? x->final_obs : nullptr; const uint8_t* x_code = x ? x->prob_code : nullptr;
    const bool any_out = a->obs || a->reward || a->terminated || a->truncated || x_fin || x_code;
    const bool strides = (a->sample_actions || a->act_stride % e == 0) && (!any_out || a->out_stride % e == 0);
    return strides && aligned(a->act_a, e) && aligned(a->act_b, e) && aligned(a->reward, e) &&
           aligned(a->terminated, e) && aligned(a->truncated, e) && aligned(a->obs, 2 * e) && aligned(x_code, e) && aligned(x_fin, 2 * e) &&
           aligned(a->return_sum, 4 * e) && aligned(a->episode_count, 4 * e);
}

// the byte-parallel rollout: every pitch that fits the byte arithmetic, slip 0 or an exact integer slip decision
// (a lane count that is not a multiple of 4: the byte-parallel kernel over the first n & ~3 lanes, the one to three
// left over through the per-lane kernel on the same ticks, like batched_step's ragged tail)
bool rollout_takes_swar(const soccer_handle* h, const soccer_rollout_args* a, const soccer_rollout_extra* x) {
    return h->swar_ok && (!h->slip || h->slip_swar_ok) && h->P.n >= 4ull && ((h->P.lane_offset + h->P.first) & 3ull) == 0ull &&
           rollout_vec_ok(a, x, 4) && h->rollout_pref != 1;
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
    int E = h->E;
    while (E > 1 && !rollout_vec_ok(a, x, E)) E = E == 4 ? 1 : E / 2;
    const bool swar_roll = rollout_takes_swar(h, a, x);
    if (!hist && (!swar_roll || (h->P.n & 3ull) || a->sample_actions || h->P.policy_a || h->P.policy_b || x_fin || x_code))
        return fail(h, SOCCER_E_STATE, "rollout without statistics: not the shape of a fused run of captured steps");
    // one launch covers at most kChunk steps (per-thread episode counters are 16 bit wide); the tick
    // sequence of consecutive launches is contiguous, so chunking does not change any result
    constexpr int kChunk = 4096;
    const Rules& R0 = h->rules;
    for (int s0 = 0; s0 < a->n_steps; s0 += kChunk) {
        const int ns = a->n_steps - s0 < kChunk ? a->n_steps - s0 : kChunk;
        KernelParams P = h->P;
        P.hist = hist;
        bind_tick(h, P, (uint64_t)ns);
        const long long ao = (long long)s0 * a->act_stride, oo = (long long)s0 * a->out_stride;
        RolloutIO io{ns, a->sample_actions, a->mix_a, a->mix_b, a->act_a ? a->act_a + ao : nullptr, a->act_b ? a->act_b + ao : nullptr,
                     (long long)a->act_stride, a->obs ? a->obs + oo : nullptr, a->reward ? a->reward + oo : nullptr,
                     a->terminated ? a->terminated + oo : nullptr, a->truncated ? a->truncated + oo : nullptr,
                     (long long)a->out_stride, a->return_sum, a->episode_count, x_fin ? x_fin + oo : nullptr, x_code ? x_code + oo : nullptr};
        const unsigned long long n_all = P.n, n4 = swar_roll ? (P.n & ~3ull) : 0ull;
        if (swar_roll) {
            P.n = n4;
            const bool dyn = io.sample_actions || P.policy_a || P.policy_b;
            RolloutSwar RS{P.state, P.state_stride, P.state_layout, P.first, P.n, P.lane_offset, P.tick_in, P.tick_out, P.hist, P.misuse,
                           P.policy_a, P.policy_b, P.key0, P.key1,
                           h->swar_c, h->slip_c, reinterpret_cast<const swar::Quad*>(P.sub), P.hist_mask, R0.nS, 0, 0u, 0u, h->d_slip_lut};
            const int sm = !h->slip ? 0 : (h->d_slip_lut ? 2 : 1);    // slip selection: none / threshold by threshold / by table
            size_t smem = 36 * sizeof(uint32_t);        // (the bucket table of sm == 2 is static LDS of the kernel)
            RS.tab_off = (uint32_t)(smem / sizeof(uint32_t));
            const bool fixed = P.policy_a || P.policy_b;
            // both sides sampled from mixed-policy tables whose 16-byte rows fit LDS: the shape of config 5
            // what the tables may take: the device's per-workgroup LDS limit (64 KB on CDNA3, 160 KB on gfx950 — never a literal)
            // minus the action staging area that is added below and the static bucket table of sm == 2
            const size_t staging = io.sample_actions ? 0 : 16 * kBlock * sizeof(uint32_t) + 16;
            const size_t lds_cap = h->lds_limit > staging + (sm == 2 ? kSlipLutWords * sizeof(uint32_t) : 0)
                                 ? h->lds_limit - staging - (sm == 2 ? kSlipLutWords * sizeof(uint32_t) : 0) : 0;
            const bool both_mix = dyn && !fixed && io.sample_actions && io.mix_a && io.mix_b &&
                                  smem + (size_t)R0.nS * sizeof(uint4) <= lds_cap;
            if (both_mix) { RS.lds_tables = 1; smem += (size_t)R0.nS * sizeof(uint4); }
            else if (dyn && (io.mix_a || io.mix_b || fixed)) {
                const size_t need = smem + 2 * (size_t)R0.nS * sizeof(uint2) + 2 * (((size_t)R0.nS + 15) & ~size_t(15));
                if (need <= lds_cap) { RS.lds_tables = 1; smem = need; }     // else: the tables stay in global memory
            }
            if (!io.sample_actions) {        // action streams are staged through LDS: 16 dwords per thread
                smem = (smem + 15) & ~size_t(15);
                RS.act_off = (uint32_t)(smem / sizeof(uint32_t));
                smem += 16 * kBlock * sizeof(uint32_t);
            }
            // The kernel's byte offsets are 32-bit: a handle beyond kSwarLaunchLanes lanes is rolled out part by part (lanes never
            // interact), every part over the same ticks, each handed its piece of every stream; the last one publishes the tick.
            const RolloutSwar RS0 = RS; const RolloutIO io0 = io;
            soccer_rollout_shape_info sh{};             // soccer_rollout_shape: what this chunk launches
            sh.kernel = SOCCER_ROLLOUT_BYTE_PARALLEL; sh.tail = n4 < n_all; sh.slip_selection = sm; sh.small_pitch = h->swar_c.small ? 1 : 0;
            sh.full = (io.final_obs || io.prob_code) ? 1 : 0; sh.dynamic_lds_bytes = smem;
            sh.table_placement = !(dyn && (io.mix_a || io.mix_b || fixed)) ? SOCCER_TABLES_NONE : RS.lds_tables ? SOCCER_TABLES_LDS : SOCCER_TABLES_GLOBAL;
            for (unsigned long long c0 = 0; c0 < n4; c0 += h->swar_launch_lanes) {
            const unsigned long long cn = std::min<unsigned long long>(h->swar_launch_lanes, n4 - c0);
            RS = RS0; io = io0;
            RS.state = RS0.state + P.first + c0; RS.first = 0ull; RS.n = cn; RS.lane_offset = RS0.lane_offset + P.first + c0;
            if (c0 + cn < n4) RS.tick_out = nullptr;
            const unsigned long long lane0 = P.first + c0;
            io.act_a = off(io0.act_a, lane0); io.act_b = off(io0.act_b, lane0); io.obs = off(io0.obs, lane0); io.reward = off(io0.reward, lane0);
            io.terminated = off(io0.terminated, lane0); io.truncated = off(io0.truncated, lane0);
            io.return_sum = off(io0.return_sum, lane0); io.episode_count = off(io0.episode_count, lane0);
            io.final_obs = off(io0.final_obs, lane0); io.prob_code = off(io0.prob_code, lane0);
            const uint64_t groups = cn >> 2;
            uint64_t blocks = (groups + kBlock - 1) / kBlock;
            if (blocks > (uint64_t)h->grid_cap) blocks = h->grid_cap;
            const dim3 g((unsigned)blocks), bl(kBlock);
#define LAUNCH_T(DV, SV, GV, FV, TV) do { if (smem > 48 * 1024) HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&rollout_swar_kernel<DV, SV, GV, FV, TV>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)); \
                                          hipLaunchKernelGGL((rollout_swar_kernel<DV, SV, GV, FV, TV>), g, bl, smem, h->stream, RS, io); } while (0)
            // (the shape without statistics exists for streamed actions and the plain result streams only: checked on entry)
#define LAUNCH_F(DV, SV, GV, FV) do { if constexpr (kUnreadShape<DV, FV>) { if (!hist) LAUNCH_T(DV, SV, GV, FV, false); else LAUNCH_T(DV, SV, GV, FV, true); } \
                                      else LAUNCH_T(DV, SV, GV, FV, true); } while (0)
#define LAUNCH_G(DV, SV, GV) do { if (io.final_obs || io.prob_code) LAUNCH_F(DV, SV, GV, true); else LAUNCH_F(DV, SV, GV, false); } while (0)
#define LAUNCH_S(DV, SV) do { if (h->swar_c.small) LAUNCH_G(DV, SV, 1); else LAUNCH_G(DV, SV, 0); } while (0)
            // the action source as a compile-time shape (rollout_swar_group): streams / sampled uniformly / both sides from
            // mixed-policy tables / single-agent A or B / anything else
            const int dm = !dyn ? 0 : (!fixed && io.sample_actions && !io.mix_a && !io.mix_b) ? 1
                                : both_mix ? 2
                                : (!io.sample_actions && P.policy_a && !P.policy_b && io.act_b) ? 4
                                : (!io.sample_actions && P.policy_b && !P.policy_a && io.act_a) ? 5 : 3;
#define LAUNCH_D(SV) do { if (dm == 0) LAUNCH_S(0, SV); else if (dm == 1) LAUNCH_S(1, SV); else if (dm == 2) LAUNCH_S(2, SV); \
                          else if (dm == 4) LAUNCH_S(4, SV); else if (dm == 5) LAUNCH_S(5, SV); else LAUNCH_S(3, SV); } while (0)
            if (sm == 0) LAUNCH_D(0); else if (sm == 1) LAUNCH_D(1); else LAUNCH_D(2);
            note_kernel(h);
            sh.action_source = dm; sh.parts += 1;
#undef LAUNCH_D
#undef LAUNCH_S
#undef LAUNCH_G
#undef LAUNCH_F
#undef LAUNCH_T
            }
            if (n4 < n_all) {
                KernelParams Q = h->P;
                Q.hist = hist;
                Q.tick_in = P.tick_in; Q.tick_out = nullptr;      // the main launch publishes the tick
                Q.first = n4; Q.n = n_all - n4;
                launch_rollout<1>(h, Q, io0);           // (io0: the loop above left `io` offset to its last part; the per-lane kernel indexes by absolute lane)
            }
            h->last_rollout = sh;
        } else {
            switch (E) {
                case 8: launch_rollout<8>(h, P, io); break;
                case 4: launch_rollout<4>(h, P, io); break;
                default: launch_rollout<1>(h, P, io); break;
            }
            const bool tables = P.policy_a || P.policy_b || (io.sample_actions && (io.mix_a || io.mix_b));
            soccer_rollout_shape_info sh{};
            sh.kernel = SOCCER_ROLLOUT_PER_LANE; sh.action_source = (io.sample_actions || P.policy_a || P.policy_b) ? 3 : 0;
            sh.slip_selection = h->slip ? 1 : 0; sh.full = (io.final_obs || io.prob_code) ? 1 : 0;
            sh.table_placement = tables ? SOCCER_TABLES_GLOBAL : SOCCER_TABLES_NONE; sh.parts = 1; sh.dynamic_lds_bytes = h->smem_bytes;
            h->last_rollout = sh;
        }
        h->last_rollout.chunks = (a->n_steps + kChunk - 1) / kChunk;
        HIP_TRY(h, hipGetLastError());
    }
    return SOCCER_OK;
}
