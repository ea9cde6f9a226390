// soccer_dispatch.hpp — run-time values to compile-time constants, once: a launcher nests these around ONE hipLaunchKernelGGL or
// hipFuncSetAttribute inside generic lambdas, so the order of a kernel's template arguments is written where the kernel is
// named and nowhere else.  A lambda's parameter is a std::integral_constant; inside nested lambdas read it as
// decltype(v)::value.  Combinations that must not be instantiated are cut with `if constexpr` in the innermost lambda, which
// returns whether it launched.
// Also: the facts a handle contributes to soccer_launch_plan.hpp's plans.  Internal, host side.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "soccer_handle.hpp"
#include "soccer_launch_plan.hpp"

#pragma GCC visibility push(hidden)

// f(std::bool_constant<v>)
template <class F>
static inline auto with_flag(bool v, F&& f) { return v ? f(std::true_type{}) : f(std::false_type{}); }

// f(std::integral_constant<int, V>) for the listed V that equals v.  A value that is not listed calls nothing and gives a
// value-initialised result: the launchers' lambdas return whether they launched, so such a call ends in NOT_COMPILED
template <int V, int... Rest, class F>
static inline auto with_value(int v, F&& f) {
    if (v == V) return f(std::integral_constant<int, V>{});
    if constexpr (sizeof...(Rest) == 0) return decltype(f(std::integral_constant<int, V>{})){};
    else return with_value<Rest...>(v, f);
}

// what a launcher answers when its lambda launched nothing: the plan named template values that are cut by `if constexpr`
// or not listed.  No plan does (tests/test_launch_plan_host.py); an edit of a plan that does must not skip a launch silently
#define NOT_COMPILED(h, what) fail((h), SOCCER_E_STATE, "%s: the launch plan names an instantiation that is not compiled", (what))

// f(slip, lut_lds) with the handle's two shape bits as compile-time constants: f names the kernel template
template <class F>
static inline auto with_shape(const soccer_handle* h, F&& f) {
    return with_flag(h->slip, [&](auto slip) { return with_flag(h->lut_lds, [&](auto lds) { return f(slip, lds); }); });
}

// a creation: the rule tables of a large pitch need more than the default LDS
template <class K>
static inline hipError_t raise_lds_limit(const soccer_handle* h, K* kernel) {
    return h->smem_bytes > 48 * 1024 ? hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                           (int)h->smem_bytes) : hipSuccess;
}

// what the handle contributes to a plan
static inline HandleFacts handle_facts(const soccer_handle* h) {
    HandleFacts f;
    f.swar_ok = h->swar_ok; f.slip = h->slip; f.slip_swar_ok = h->slip_swar_ok;
    f.slip_lut = h->d_slip_lut != nullptr; f.slip_step_lut = h->d_slip_step_lut != nullptr;
    f.small = h->swar_c.small != 0u; f.wide = h->P.state_layout == kStateWide; f.lut_lds = h->lut_lds;
    f.policy_a = h->P.policy_a != nullptr; f.policy_b = h->P.policy_b != nullptr;
    f.step_stats = h->P.step_stats != 0u; f.slip_int_one = h->P.slip_int == 1u;
    f.stream_actions = (h->cfg.flags & SOCCER_F_STREAM_ACTIONS) != 0;
    f.capturing = h->capturing; f.worklist = h->d_worklist != nullptr;
    f.E = h->E; f.rollout_pref = h->rollout_pref; f.nS = h->rules.nS;
    f.lane_phase = (unsigned)((h->P.lane_offset + h->P.first) & 3ull);
    f.smem_bytes = h->smem_bytes; f.lds_limit = h->lds_limit; f.n = h->P.n;
    return f;
}

// dword (e = 4) or wider I/O needs every stream aligned to e of its elements and both strides multiples of e
static inline bool rollout_vec_ok(const soccer_rollout_args* a, const soccer_rollout_extra* x, int e) {
    const uint16_t* x_fin = x ? x->final_obs : nullptr; const uint8_t* x_code = x ? x->prob_code : nullptr;
    const bool any_out = a->obs || a->reward || a->terminated || a->truncated || x_fin || x_code;
    const bool strides = (a->sample_actions || a->act_stride % e == 0) && (!any_out || a->out_stride % e == 0);
    return strides && aligned(a->act_a, e) && aligned(a->act_b, e) && aligned(a->reward, e) &&
           aligned(a->terminated, e) && aligned(a->truncated, e) && aligned(a->obs, 2 * e) && aligned(x_code, e) && aligned(x_fin, 2 * e) &&
           aligned(a->return_sum, 4 * e) && aligned(a->episode_count, 4 * e);
}

// what a rollout's arguments contribute to its plan; `hist`: somebody reads its episode statistics
static inline RolloutCall rollout_call(const soccer_rollout_args* a, const soccer_rollout_extra* x, bool hist) {
    RolloutCall c;
    c.sample_actions = a->sample_actions != 0; c.mix_a = a->mix_a != nullptr; c.mix_b = a->mix_b != nullptr;
    c.act_a = a->act_a != nullptr; c.act_b = a->act_b != nullptr;
    c.full = x && (x->final_obs || x->prob_code);
    c.hist = hist;
    c.io_width = rollout_vec_ok(a, x, 8) ? 8 : rollout_vec_ok(a, x, 4) ? 4 : 1;
    return c;
}

#pragma GCC visibility pop
