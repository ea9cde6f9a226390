// soccer_launch_plan.hpp — which kernel instantiation batched_step, batched_rollout and batched_reset launch, decided once and
// apart from the launch: what the handle and the call contribute go in as plain facts, a plan comes out, and the launchers
// (soccer_step.hip, soccer_rollout.hip, soccer_hip.hip) take every branch from it: a launch of these three calls takes its
// template values from a plan and from nowhere else.  Plain C++ with no HIP in it, and pure; tests/host/launch_plan_host.cpp compiles it for the CPU tests.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/soccer_hip.h"

namespace soccer {

// what the handle contributes to every plan (soccer_create fixes all of it but `capturing` and `worklist`)
struct HandleFacts {
    bool swar_ok, slip, slip_swar_ok;   // the pitch fits the byte arithmetic; slip_prob != 0; ... with an exact integer decision
    bool slip_lut, slip_step_lut;       // the table forms of the slip selection exist: the rollout's, the single step's
    bool small, wide;                   // swar::Consts::small (GEO = 1); six state streams, not the three packed ones
    bool lut_lds;                       // the per-lane kernels stage the observation table in LDS
    bool policy_a, policy_b, step_stats, slip_int_one, stream_actions;
    bool capturing, worklist;           // a graph is being captured; the exact walk's work list exists
    int E, rollout_pref, nS;            // envs_per_thread (1, 4, 8); SOCCER_ROLLOUT; observation indices
    unsigned lane_phase;                // (lane_offset + first) & 3
    size_t smem_bytes, lds_limit;       // dynamic LDS of the per-lane kernels; what a workgroup of the device may be given
    unsigned long long n;
};

// ---- batched_step ------------------------------------------------------------------------------------------------------------
struct StepCall {
    bool dword_io;                      // every stream given is aligned for dword I/O (bytes 4, uint16 8, float 16)
    bool u_step, u_reset, u_aligned16;  // caller-supplied uniforms: given; both 16-byte aligned (a stream not given is)
    bool last_return, last_return_aligned4;
    bool full, gym;                     // prob_code / final_obs asked for; reward_a_f32 / reward_b_f32 / finished asked for
};

enum StepFamily : int { kStepNone = 0, kStepSwar = 1, kStepLane = 2, kStepHot = 3 };

// one launch_step: the family and its template values (the others are zero)
struct StepLaunch {
    int family;
    int out, slipm, geo; bool policy, expl;         // step_kernel_swar<OUT, SLIPM, POLICY, GEO, EXPL, wide ? kStateWide : kStatePacked>
    bool explicit_u, vec, shared;                   // step_kernel<slip, EXPLICIT_U, VEC, SHARED>
    bool int_only;                                  // step_kernel_hot<slip, INT_ONLY>
    bool slip, wide;
    bool exact_tail;                                // SLIPM == 3: step_kernel<true, true, true, true> walks the listed groups after every part
    bool act_stream;                                // bit 0 of the byte-parallel kernel's lane count: the action-load policy
};

// the dword-aligned lanes [0, n4) in one launch_step, the ragged rest (or everything) in another on the same tick
struct StepPlan {
    unsigned long long n4;
    StepLaunch main, rest;
};

// one launch_step over `n` lanes; `listable`: a work list exists or may be allocated by this call
inline StepLaunch plan_step_part(const HandleFacts& f, const StepCall& c, bool vec, unsigned long long n, bool listable) {
    StepLaunch L{};
    const bool policy = f.policy_a || f.policy_b;
    const bool explicit_u = c.u_step || c.u_reset || policy;            // generic kernel
    const bool shared = f.lane_phase == 0u;
    const bool policy_only = explicit_u && !c.u_step && !c.u_reset;     // fixed-policy handle, Philox draws
    const bool byte_io = vec && shared && f.swar_ok && c.last_return_aligned4;
    const bool swar_fit = byte_io && (!f.slip || f.slip_swar_ok);
    // caller-supplied uniforms at slip_prob == 0: floor(4u) is the reference's decision for any double (step_kernel_swar, EXPL)
    const bool expl = explicit_u && !policy_only && !f.slip && c.u_aligned16;
    // ... and at slip_prob > 0 the float64 decision against the nominal thresholds (SLIPM = 3); the groups it cannot decide safely go
    // to the per-lane kernel's exact walk through a work list (one extra small launch per part)
    const bool expl_slip = explicit_u && !policy_only && f.slip && c.u_step && c.u_aligned16 && byte_io && (n >> 2) < 0xffffffffull && listable;
    L.slip = f.slip;
    if (((policy_only || !explicit_u || expl) && swar_fit) || expl_slip) {
        // the byte-parallel kernel.  Which outputs the launch needs decides OUT: 0 the four result streams, 1 + the gym floats /
        // finished / last_return, 2 + final_obs / prob_code / episode histogram
        L.family = kStepSwar;
        L.out = (c.full || f.step_stats) ? 2 : (c.gym || c.last_return) ? 1 : 0;
        L.expl = expl_slip || expl;
        L.slipm = expl_slip ? 3 : (expl || !f.slip) ? 0 : f.slip_step_lut ? 2 : 1;
        L.policy = policy;
        // six-stream handles that fit the byte arithmetic are host-mapped facade handles, tall pitches and SOCCER_STATE_LAYOUT=wide:
        // nobody times them, so they take the arithmetic geometry (GEO = 0, right for every pitch) instead of mirroring every shape
        L.wide = f.wide;
        L.geo = (!f.wide && f.small) ? 1 : 0;
        L.exact_tail = expl_slip;
        L.act_stream = f.stream_actions;
    } else if (explicit_u) {    // caller-supplied uniforms (facade, tests) and fixed-policy handles beyond the byte arithmetic
        L.family = kStepLane; L.explicit_u = true; L.vec = L.shared = vec && shared;
    } else if (vec && shared && !c.full && !c.gym && !c.last_return && !f.step_stats) {
        // step_kernel_hot has no code for prob_code / final_obs / last_return / the gym outputs / step stats, step_kernel writes them
        L.family = kStepHot; L.int_only = f.slip && f.slip_int_one;
    } else {
        L.family = kStepLane; L.vec = vec; L.shared = vec && shared;
    }
    return L;
}

// `worklist_refused`: the allocation of the work list failed in this call, plan without it
inline StepPlan plan_step(const HandleFacts& f, const StepCall& c, bool worklist_refused = false) {
    StepPlan S{};
    const bool listable = f.worklist || (!f.capturing && !worklist_refused);    // (no allocation inside a capture)
    S.n4 = (f.E != 1 && c.dword_io) ? (f.n & ~3ull) : 0ull;
    if (S.n4) S.main = plan_step_part(f, c, true, S.n4, listable);
    if (S.n4 < f.n) S.rest = plan_step_part(f, c, false, f.n - S.n4, listable);
    return S;
}

// ---- batched_rollout ---------------------------------------------------------------------------------------------------------
struct RolloutCall {
    bool sample_actions, mix_a, mix_b, act_a, act_b;
    bool full;                          // final_obs / prob_code asked for
    bool hist;                          // somebody reads the episode statistics (not so: a fused run of captured steps without step statistics)
    int io_width;                       // 8, 4 or 1: elements to which every stream given and both strides are aligned
};

constexpr size_t kPlanBlock = 256;                      // kBlock
constexpr size_t kPlanSlipLutBytes = (4096 + 40) * 4;   // kSlipLutWords dwords: the static bucket table of sm == 2
constexpr size_t kPlanSlipRowBytes = 36 * 4;            // the slip rows every byte-parallel rollout stages

struct RolloutPlan {
    bool refused;                       // "rollout without statistics: not the shape of a fused run of captured steps"
    bool swar;                          // rollout_swar_kernel<dm, sm, geo, full, stats> over n4 lanes; else rollout_kernel<E, slip, lut_lds, dyn> over all
    int E; bool dyn, slip, lut_lds;     // the per-lane kernel's (the tail's: E = 1)
    int dm, sm, geo; bool full, stats;
    bool lds_tables; uint32_t tab_off, act_off;
    size_t smem;                        // dynamic LDS of the main launch
    int table_placement;
    unsigned long long n4;              // lanes of the byte-parallel launches; the per-lane tail takes the rest
    bool tail;
};

// would a rollout with these arguments take rollout_swar_kernel?  (A lane count that is not a multiple of 4: the byte-parallel
// kernel over the first n & ~3 lanes, the one to three left over through the per-lane kernel on the same ticks.)
inline bool rollout_swar_ok(const HandleFacts& f, const RolloutCall& c) {
    return f.swar_ok && (!f.slip || f.slip_swar_ok) && f.n >= 4ull && f.lane_phase == 0u && c.io_width >= 4 && f.rollout_pref != 1;
}

inline RolloutPlan plan_rollout(const HandleFacts& f, const RolloutCall& c) {
    RolloutPlan R{};
    const bool fixed = f.policy_a || f.policy_b;
    R.swar = rollout_swar_ok(f, c);
    R.dyn = c.sample_actions || fixed;      // some action is produced in the kernel (sampling, mixed policy, fixed policy)
    R.full = c.full; R.slip = f.slip; R.lut_lds = f.lut_lds;
    R.refused = !c.hist && (!R.swar || (f.n & 3ull) || R.dyn || c.full);
    const bool tables = fixed || (c.sample_actions && (c.mix_a || c.mix_b));
    if (!R.swar) {
        R.E = f.E < c.io_width ? f.E : c.io_width;
        R.smem = f.smem_bytes; R.stats = true;
        R.table_placement = tables ? SOCCER_TABLES_GLOBAL : SOCCER_TABLES_NONE;
        return R;
    }
    R.E = 1; R.n4 = f.n & ~3ull; R.tail = R.n4 < f.n;
    R.sm = !f.slip ? 0 : (f.slip_lut ? 2 : 1);      // slip selection: none / threshold by threshold / by table
    R.geo = f.small ? 1 : 0;
    size_t smem = kPlanSlipRowBytes;                // (the bucket table of sm == 2 is static LDS of the kernel)
    R.tab_off = (uint32_t)(smem / sizeof(uint32_t));
    // what the tables may take: the device's per-workgroup LDS limit (64 KB on CDNA3, 160 KB on gfx950 — never a literal)
    // minus the action staging area that is added below and the static bucket table of sm == 2
    const size_t staging = c.sample_actions ? 0 : 16 * kPlanBlock * sizeof(uint32_t) + 16;
    const size_t taken = staging + (R.sm == 2 ? kPlanSlipLutBytes : 0);
    const size_t lds_cap = f.lds_limit > taken ? f.lds_limit - taken : 0;
    // both sides sampled from mixed-policy tables whose 16-byte rows fit LDS: the shape of config 5
    const bool both_mix = R.dyn && !fixed && c.sample_actions && c.mix_a && c.mix_b && smem + (size_t)f.nS * 16 <= lds_cap;
    if (both_mix) { R.lds_tables = true; smem += (size_t)f.nS * 16; }
    else if (R.dyn && (c.mix_a || c.mix_b || fixed)) {
        const size_t need = smem + 2 * (size_t)f.nS * 8 + 2 * (((size_t)f.nS + 15) & ~size_t(15));
        if (need <= lds_cap) { R.lds_tables = true; smem = need; }      // else: the tables stay in global memory
    }
    if (!c.sample_actions) {            // action streams are staged through LDS: 16 dwords per thread
        smem = (smem + 15) & ~size_t(15);
        R.act_off = (uint32_t)(smem / sizeof(uint32_t));
        smem += 16 * kPlanBlock * sizeof(uint32_t);
    }
    R.smem = smem;
    // the action source as a compile-time shape (rollout_swar_group): streams / sampled uniformly / both sides from
    // mixed-policy tables / single-agent A or B / anything else
    R.dm = !R.dyn ? 0 : (!fixed && c.sample_actions && !c.mix_a && !c.mix_b) ? 1
                      : both_mix ? 2
                      : (!c.sample_actions && f.policy_a && !f.policy_b && c.act_b) ? 4
                      : (!c.sample_actions && f.policy_b && !f.policy_a && c.act_a) ? 5 : 3;
    R.stats = c.hist || R.dm != 0 || R.full;        // the shape without statistics: streamed actions and the plain result streams only
    R.table_placement = !(R.dyn && (c.mix_a || c.mix_b || fixed)) ? SOCCER_TABLES_NONE : R.lds_tables ? SOCCER_TABLES_LDS : SOCCER_TABLES_GLOBAL;
    return R;
}

// may a captured step be part of a fused run at all (`r`: the step as a rollout of one step)?  Alone its plan is then the
// byte-parallel kernel with OUT 0 or, with step statistics, OUT 2 for the histogram only.  This asks the ROLLOUT's plan whether a
// run of such steps is byte-parallel; that plan_step agrees on every combination of the facts is what
// tests/test_launch_plan_host.py holds the two to (its step sweep: fusable implies that family and those OUT values)
inline bool step_fusable(const HandleFacts& f, const StepCall& c, const RolloutCall& r) {
    if (f.policy_a || f.policy_b || f.E == 1 || (f.n & 3ull)) return false;
    if (c.u_step || c.u_reset || c.gym || c.last_return || c.full) return false;
    return rollout_swar_ok(f, r);
}

// soccer_rollout_shape's answer for one chunk of this plan; the launch loops count `parts` (of the byte-parallel kernel) and `chunks`
inline soccer_rollout_shape_info rollout_shape_of(const HandleFacts& f, const RolloutPlan& R, int parts, int chunks) {
    soccer_rollout_shape_info sh{};
    sh.kernel = R.swar ? SOCCER_ROLLOUT_BYTE_PARALLEL : SOCCER_ROLLOUT_PER_LANE;
    sh.tail = R.tail ? 1 : 0;
    sh.action_source = R.swar ? R.dm : (R.dyn ? 3 : 0);
    sh.slip_selection = R.swar ? R.sm : (f.slip ? 1 : 0);
    sh.small_pitch = R.swar ? R.geo : 0;
    sh.full = R.full ? 1 : 0;
    sh.table_placement = R.table_placement;
    sh.parts = R.swar ? parts : 1; sh.chunks = chunks;
    sh.dynamic_lds_bytes = R.smem;
    return sh;
}

// ---- batched_reset -----------------------------------------------------------------------------------------------------------
struct ResetCall {
    bool mask, u_reset, dword_io;       // dword_io: mask 4-byte and obs 8-byte aligned (a stream not given is)
};

// reset_kernel_swar<masked, slip> over the first n4 lanes (Philox draws, dword-aligned streams), reset_kernel<lut_lds, slip>
// over whatever is left — a ragged tail, or everything — on the same tick
struct ResetPlan {
    unsigned long long n4;
    bool masked, slip, lut_lds;
};

inline ResetPlan plan_reset(const HandleFacts& f, const ResetCall& c) {
    ResetPlan R{};
    if (f.swar_ok && !c.u_reset && f.E != 1 && f.lane_phase == 0u && c.dword_io) R.n4 = f.n & ~3ull;
    R.masked = c.mask; R.slip = f.slip; R.lut_lds = f.lut_lds;
    return R;
}

}  // namespace soccer
