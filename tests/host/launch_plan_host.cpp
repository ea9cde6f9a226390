// Host build of the kernel choice of batched_step / batched_rollout / batched_reset
// (gym_soccer_littman94_amd/csrc/soccer_launch_plan.hpp) for tests/test_launch_plan_host.py and tests/test_gpu_launch_plan.py:
// rows of facts in, rows of plans out, every value an int64.  The column orders are those of tests/launch_plan_cases.py.
// Test infrastructure; not part of libsoccer_hip.so.
// As a sanitized program of its own (a few thousand plans over mixed facts, prints a checksum):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DLAUNCH_PLAN_MAIN -o launch_plan_main tests/host/launch_plan_host.cpp && ./launch_plan_main
#include <cstdint>

#include "../../gym_soccer_littman94_amd/csrc/soccer_launch_plan.hpp"

using namespace soccer;
typedef long long i64;

enum { kHandleCols = 22, kStepCols = 9, kRolloutCols = 10, kResetCols = 3, kLaunchCols = 14 };

static HandleFacts handle_of(const i64* v) {
    HandleFacts f{};
    f.swar_ok = v[0]; f.slip = v[1]; f.slip_swar_ok = v[2]; f.slip_lut = v[3]; f.slip_step_lut = v[4]; f.small = v[5]; f.wide = v[6];
    f.lut_lds = v[7]; f.policy_a = v[8]; f.policy_b = v[9]; f.step_stats = v[10]; f.slip_int_one = v[11]; f.stream_actions = v[12];
    f.capturing = v[13]; f.worklist = v[14]; f.E = (int)v[15]; f.rollout_pref = (int)v[16]; f.nS = (int)v[17];
    f.lane_phase = (unsigned)v[18]; f.smem_bytes = (size_t)v[19]; f.lds_limit = (size_t)v[20]; f.n = (unsigned long long)v[21];
    return f;
}

static i64* put_launch(i64* o, const StepLaunch& L) {
    const i64 v[kLaunchCols] = {L.family, L.out, L.slipm, L.geo, L.policy, L.expl, L.explicit_u, L.vec, L.shared, L.int_only, L.slip, L.wide,
                                L.exact_tail, L.act_stream};
    for (int i = 0; i < kLaunchCols; ++i) *o++ = v[i];
    return o;
}

// in [rows][22 + 9]: the handle, then dword_io, u_step, u_reset, u_aligned16, last_return, last_return_aligned4, full, gym,
// worklist_refused.  out [rows][1 + 14 + 14 + 1]: n4, the main launch, the rest's, step_fusable (the step as a rollout of one step,
// its streams aligned to 4 elements exactly when dword_io)
extern "C" void plan_step_host(long rows, const i64* in, i64* out) {
    for (long r = 0; r < rows; ++r, in += kHandleCols + kStepCols) {
        const HandleFacts f = handle_of(in);
        const i64* v = in + kHandleCols;
        StepCall c{};
        c.dword_io = v[0]; c.u_step = v[1]; c.u_reset = v[2]; c.u_aligned16 = v[3]; c.last_return = v[4]; c.last_return_aligned4 = v[5];
        c.full = v[6]; c.gym = v[7];
        const StepPlan S = plan_step(f, c, v[8] != 0);
        *out++ = (i64)S.n4;
        out = put_launch(put_launch(out, S.main), S.rest);
        RolloutCall one{};
        one.act_a = one.act_b = one.hist = true; one.io_width = c.dword_io ? 4 : 1;
        *out++ = step_fusable(f, c, one);
    }
}

// in [rows][22 + 10]: the handle, then sample_actions, mix_a, mix_b, act_a, act_b, full, hist, io_width, parts, chunks.
// out [rows][18 + 10]: the plan (refused, swar, E, dyn, dm, sm, geo, full, stats, lds_tables, tab_off, act_off, smem,
// table_placement, n4, tail, slip, lut_lds), then the plan read as soccer_rollout_shape_info (kernel, tail, action_source, slip_selection,
// small_pitch, full, table_placement, parts, chunks, dynamic_lds_bytes)
extern "C" void plan_rollout_host(long rows, const i64* in, i64* out) {
    for (long r = 0; r < rows; ++r, in += kHandleCols + kRolloutCols) {
        const HandleFacts f = handle_of(in);
        const i64* v = in + kHandleCols;
        RolloutCall c{};
        c.sample_actions = v[0]; c.mix_a = v[1]; c.mix_b = v[2]; c.act_a = v[3]; c.act_b = v[4]; c.full = v[5]; c.hist = v[6];
        c.io_width = (int)v[7];
        const RolloutPlan R = plan_rollout(f, c);
        const soccer_rollout_shape_info sh = rollout_shape_of(f, R, (int)v[8], (int)v[9]);
        const i64 o[28] = {R.refused, R.swar, R.E, R.dyn, R.dm, R.sm, R.geo, R.full, R.stats, R.lds_tables, R.tab_off, R.act_off, (i64)R.smem,
                           R.table_placement, (i64)R.n4, R.tail, R.slip, R.lut_lds,
                           sh.kernel, sh.tail, sh.action_source, sh.slip_selection, sh.small_pitch, sh.full, sh.table_placement, sh.parts,
                           sh.chunks, (i64)sh.dynamic_lds_bytes};
        for (int i = 0; i < 28; ++i) *out++ = o[i];
    }
}

// in [rows][22 + 3]: the handle, then mask, u_reset, dword_io.  out [rows][4]: n4, masked, slip, lut_lds
extern "C" void plan_reset_host(long rows, const i64* in, i64* out) {
    for (long r = 0; r < rows; ++r, in += kHandleCols + kResetCols) {
        const i64* v = in + kHandleCols;
        const ResetPlan R = plan_reset(handle_of(in), ResetCall{v[0] != 0, v[1] != 0, v[2] != 0});
        *out++ = (i64)R.n4; *out++ = R.masked; *out++ = R.slip; *out++ = R.lut_lds;
    }
}

#ifdef LAUNCH_PLAN_MAIN
#include <cstdio>
int main() {
    i64 in[kHandleCols + kRolloutCols], out[30], sum = 0;
    for (i64 k = 0; k < 4096; ++k) {
        for (int i = 0; i < kHandleCols + kRolloutCols; ++i) in[i] = (k >> (i % 12)) & 1;
        in[15] = (k & 1) ? 4 : (k & 2) ? 8 : 1; in[17] = 761 + 97 * (k & 63); in[19] = 4096; in[20] = 64 * 1024 << (k & 1); in[21] = 3 + (k & 7);
        in[kHandleCols + 7] = (k & 4) ? 4 : 1;
        plan_step_host(1, in, out); sum += out[0] + out[1];
        plan_rollout_host(1, in, out); sum += out[12];
        plan_reset_host(1, in, out); sum += out[0];
    }
    std::printf("%lld\n", sum);
    return 0;
}
#endif
