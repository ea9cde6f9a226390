// soccer_rollout_kernels.hpp — the fused T-step kernels: rollout_kernel, rollout_swar_kernel.
// Included by soccer_rollout.hip only: every kernel is emitted by exactly one translation unit.
#pragma once
#include "soccer_kernels.hpp"

namespace soccer {

// =================================================================================================
// batched_rollout: T fused steps, state in registers, actions streamed in, trajectories streamed out
// =================================================================================================
// DYN = false: both action streams come from memory (the trajectory collector); the code for in-kernel
// sampling, mixed policies and the fixed-policy gather is compiled out.
template <int E, bool SLIP, bool DYN>
__device__ __forceinline__ void rollout_group(const Tables& T, const KernelParams& P, const RolloutIO& IO,
                                              unsigned long long i0, unsigned long long tick0,
                                              HistAcc<false>& hist, bool& any_misuse) {
    LaneVec<E> S; S.load(P, i0);
    int32_t ret[E], eps[E];
    uint32_t nonzero = 0u;                  // number of steps of this thread's lanes that carried a reward
#pragma unroll
    for (int j = 0; j < E; ++j) { ret[j] = 0; eps[j] = 0; }
    PackB<E> aa, ab; aa.clear(); ab.clear();
    const bool sample = DYN && IO.sample_actions;
    uint32_t bad_act = 0u;
    if (!sample) {
        if (!DYN || IO.act_a) aa.load_nt(IO.act_a, i0);
        if (!DYN || IO.act_b) ab.load_nt(IO.act_b, i0);
        bad_act |= canon_pack(aa) | canon_pack(ab);
    }
    // the observation of the current tuple is carried along when an action depends on it
    const bool fixed = DYN && (P.policy_a != nullptr || P.policy_b != nullptr ||    // single-agent mode
                               (sample && (IO.mix_a != nullptr || IO.mix_b != nullptr)));
    uint32_t s_now[E];
#pragma unroll
    for (int j = 0; j < E; ++j) s_now[j] = fixed ? obs_of(T, P, S.L[j].A, S.L[j].B, S.L[j].p) : 0u;
    for (int s = 0; s < IO.n_steps; ++s) {
        const unsigned long long tick = tick0 + (unsigned long long)s;
        PackB<E> naa = aa, nab = ab;
        if (!sample && s + 1 < IO.n_steps) {                            // prefetch the next step's actions
            if (!DYN || IO.act_a) naa.load_nt(IO.act_a + (long long)(s + 1) * IO.act_stride, i0);
            if (!DYN || IO.act_b) nab.load_nt(IO.act_b + (long long)(s + 1) * IO.act_stride, i0);
            bad_act |= canon_pack(naa) | canon_pack(nab);
        }
        uint32_t words[E], awords[E];
        lane_words<E>(P, P.lane_offset + i0, block_tick<SLIP>(tick), 0u, words);
        if (sample) lane_words<E>(P, P.lane_offset + i0, tick, 1u, awords);
        PackB<E> o_rew, o_term, o_trunc, o_code; PackH<E> o_obs, o_fin;
        o_rew.clear(); o_term.clear(); o_trunc.clear(); o_obs.clear(); o_code.clear(); o_fin.clear();
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const Draw d = draw_from_word<SLIP>(words[j], tick);
            uint32_t a = aa.get(j), b = ab.get(j);
            if (sample) {                               // two actions from one 32-bit word, 15 bits each
                const uint32_t ha = awords[j] & 0x7fffu, hb = (awords[j] >> 16) & 0x7fffu;
                a = (ha * 5u) >> 15;                    // uniform
                b = (hb * 5u) >> 15;
                if (IO.mix_a) {                         // mixed policy: first action whose cumulative threshold exceeds the draw
                    const uint2 th = *reinterpret_cast<const uint2*>(IO.mix_a + 4u * s_now[j]);
                    a = (ha >= (th.x & 0xffffu)) + (ha >= (th.x >> 16)) + (ha >= (th.y & 0xffffu)) + (ha >= (th.y >> 16));
                }
                if (IO.mix_b) {
                    const uint2 th = *reinterpret_cast<const uint2*>(IO.mix_b + 4u * s_now[j]);
                    b = (hb >= (th.x & 0xffffu)) + (hb >= (th.x >> 16)) + (hb >= (th.y & 0xffffu)) + (hb >= (th.y >> 16));
                }
            }
            if (fixed) {
                if (P.policy_a) a = (uint32_t)(uint8_t)P.policy_a[s_now[j]];
                if (P.policy_b) b = (uint32_t)(uint8_t)P.policy_b[s_now[j]];
            }
            StepResult R;
            any_misuse |= lane_step<SLIP, true>(T, P, S.L[j], a, b, d, R);
            if (DYN) s_now[j] = R.obs;
            o_obs.put(j, R.obs); o_rew.put(j, (uint32_t)R.reward & 0xffu); o_term.put(j, R.term); o_trunc.put(j, R.trunc);
            o_fin.put(j, R.final_obs); o_code.put(j, R.code);
            ret[j] += R.reward; eps[j] += (int32_t)R.finished; nonzero += (uint32_t)R.reward & 1u;
        }
        const long long off = (long long)s * IO.out_stride;
        if (IO.obs) o_obs.store_nt(IO.obs + off, i0);
        if (IO.reward) o_rew.store_nt(IO.reward + off, i0);
        if (IO.terminated) o_term.store_nt(IO.terminated + off, i0);
        if (IO.truncated) o_trunc.store_nt(IO.truncated + off, i0);
        if (IO.final_obs) o_fin.store_nt(IO.final_obs + off, i0);
        if (IO.prob_code) o_code.store_nt(IO.prob_code + off, i0);
        aa = naa; ab = nab;
    }
    S.store(P, i0);
    {
        int32_t rsum = 0; uint32_t fsum = 0u;
#pragma unroll
        for (int j = 0; j < E; ++j) { rsum += ret[j]; fsum += (uint32_t)eps[j]; }
        hist.add_totals(fsum, rsum, nonzero);
    }
    if (IO.return_sum) add_words<E>(IO.return_sum, i0, ret);
    if (IO.episode_count) add_words<E>(IO.episode_count, i0, eps);
    if (bad_act) P.misuse[1] = 1u;
}

template <int E, bool SLIP, bool LUT_LDS, bool DYN>
__global__ __launch_bounds__(kBlock) void rollout_kernel(const KernelParams P, const RolloutIO IO) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    HistAcc<false> hist; hist.init(P);
    const Tables T = stage_tables<LUT_LDS>(P, smem);
    const unsigned long long tick0 = *P.tick_in;
    if (P.tick_out) publish_tick(P, tick0, (unsigned long long)IO.n_steps);   // nullptr: the tail of a launch that already did
    const unsigned long long groups = (P.n + E - 1) / E;        // the launch covers lanes [first, first + n) of the handle
    bool any_misuse = false;
    for (unsigned long long g = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; g < groups;
         g += (unsigned long long)gridDim.x * kBlock) {
        const unsigned long long rel = g * E, i0 = P.first + rel;
        if (E == 1 || rel + E <= P.n) {
            rollout_group<E, SLIP, DYN>(T, P, IO, i0, tick0, hist, any_misuse);
        } else {
            for (unsigned long long i = rel; i < P.n; ++i)
                rollout_group<1, SLIP, DYN>(T, P, IO, P.first + i, tick0, hist, any_misuse);
        }
    }
    if (any_misuse) P.misuse[0] = 1u;
    hist.flush(P);
}

// =================================================================================================
// batched_rollout, byte-parallel: T fused steps with the four lanes of a thread packed in six registers
// =================================================================================================
// The step of soccer_swar.hpp in a loop: no rule table, no LDS transition table (so every pitch that fits the byte
// arithmetic — all golden ones up to 11x7 — and every slip whose integer decision is exact take the same kernel), no
// state-code conversion on entry / exit, frozen and goal-tuple lanes handled by the step itself.  Per step a thread
// issues one Philox block, two action dwords (prefetched a step ahead) and four result stores.
//   DYN: some action is produced in the kernel — sampled uniformly or from [nS][4] mixed-policy thresholds (config 5),
//        or looked up from a fixed int8[nS] policy (single-agent mode); these are per-lane gathers keyed by the lane's
//        current observation, which the step already produces.  The tables sit in LDS when they fit (`lds_tables`).
struct RolloutSwar {       // everything the kernel needs, and nothing else (KernelParams is twice this: SGPR spills)
    uint8_t* state; unsigned long long state_stride; uint32_t layout;      // StateLayout: read once on entry, written once on exit
    unsigned long long first, n, lane_offset;
    const unsigned long long* tick_in; unsigned long long* tick_out;
    unsigned long long* hist; unsigned int* misuse;
    const int8_t* policy_a; const int8_t* policy_b;
    uint32_t key0, key1;
    swar::Consts C; swar::SlipConsts L; const swar::Quad* sub;
    uint32_t hist_mask;
    int32_t nS; int32_t lds_tables;
    uint32_t act_off;                       // dword offset of the action staging area in dynamic LDS (16 x 256 dwords per workgroup)
    uint32_t tab_off;                       // dword offset of the mixed-policy / fixed-policy tables in dynamic LDS
    const uint32_t* slip_lut;               // SLIPM == 2: SlipTables::lut (kSlipBuckets bytes) followed by SlipTables::T
};

// where the slip selection of a byte-parallel kernel reads its thresholds: SLIPM == 1 the nine rows of quarter points
// (compared one by one, for the slips whose thresholds crowd a table bucket), SLIPM == 2 the bucket table + the ascending
// threshold list (swar::slip_select4_lut)
struct SlipSrc { const swar::Quad* sub; const uint8_t* lut; const uint32_t* T; };
constexpr int kSlipLutWords = 4096 + 40;        // = soccer::kSlipLdsWords (soccer_slip.hpp is host-only)

// A mixed-policy row holds four 16-bit cumulative thresholds t0 <= t1 <= t2 <= t3 (values 0..2^15) as two dwords; the
// action is the number of them that are <= the player's 15-bit draw h.  With `hs` = h in both halves and bit 15 set,
// (h + 0x8000) - t has bit 15 set exactly when h >= t: two packed subtractions put the four answers into the sign bits
// of bytes 1, 3, 5, 7 of an 8-byte pair, which is what v_perm_b32's selectors 8..11 replicate — one permute turns them
// into four 0xff / 0x00 bytes and one population count gives 8 x the action.
__device__ __forceinline__ uint32_t count8_le15(uint32_t hs, uint32_t tx, uint32_t ty) {
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const uint32_t x = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, hs) - __builtin_bit_cast(u16x2, tx));
    const uint32_t y = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, hs) - __builtin_bit_cast(u16x2, ty));
    return (uint32_t)__builtin_popcount(swar::perm(y, x, 0x0b0a0908u));
}
// the two 15-bit action draws of a lane's purpose-1 word w (da = w & 0x7fff, db = (w >> 16) & 0x7fff): `wm` = w with
// bits 15 and 31 forced, each half then duplicated by one byte permute
__device__ __forceinline__ uint32_t draw_a15(uint32_t wm) { return swar::perm(0u, wm, 0x01000100u); }
__device__ __forceinline__ uint32_t draw_b15(uint32_t wm) { return swar::perm(0u, wm, 0x03020302u); }

// the shapes a fused run of captured steps can take (step_can_fuse): streamed actions, the four plain result streams
template <int DYNM, bool FULL> constexpr bool kUnreadShape = DYNM == 0 && !FULL;
// which instantiations hold one half of each small-pitch byte table in a vector register across the step loop: the steady
// state of the table geometry, except the three kernels whom the five registers cost a wave of occupancy (uniformly sampled
// actions at slip 0: 7 -> 6; a fixed policy against a streamed side with the one-by-one slip selection and FULL: 5 -> 4)
template <int DYNM, int SLIPM, bool GENERAL, int GEO, bool FULL, bool STATS>
constexpr bool kHoistTables = GEO == 1 && !GENERAL && !(DYNM == 1 && SLIPM == 0 && !FULL) &&
                              !((DYNM == 4 || DYNM == 5) && SLIPM == 1 && FULL);

// the T steps of one thread's four lanes.  GENERAL = false: no lane is frozen or in a goal tuple on entry and the handle
// auto-resets, so none ever will be (the steady state): the step's code for those cases is compiled out.
// DYNM — where the actions come from: 0 both from the action streams; 1 both sampled uniformly in the kernel; 2 both
// sampled from mixed-policy tables staged in LDS as one 16-byte row per state (config 5); 4 / 5 player A / B follows its
// fixed policy and the other side's actions are streamed (single-agent mode); 3 anything else (a table on one side only,
// tables too big for LDS, a fixed policy against a sampled side ...: decided by wave-uniform run-time tests).  The common
// shapes are instantiations of their own because every optional pointer that stays live costs scalar registers, and the
// loop of the catch-all form spilled them (60-300 v_readlane_b32 per step).
// Randomness (include/soccer_hip.h): with SLIP one step/reset block per tick; without, one block per EIGHT ticks — the
// thread keeps it transposed (swar::transpose4) in p0..p3, p0 serving the current pair of ticks — which takes the Philox
// rounds from ~45 to ~6 vector instructions per step; sampled actions take the lane's word of the tick's purpose-1 block.
// STATS = false (a fused captured run of a handle without step statistics): nothing reads the episode counts, so the step
// does not make them.
template <int DYNM, int SLIPM, bool GENERAL, int GEO, bool FULL = false, bool STATS = true>
__device__ __forceinline__ void rollout_swar_group(const RolloutSwar& R, const RolloutIO& IO, const SlipSrc& slip,
                                                   const uint2* mix_a_in, const uint2* mix_b_in, const int8_t* pol_a_in, const int8_t* pol_b_in,
                                                   uint32_t* act_lds,
                                                   uint32_t i0, unsigned long long tick0, swar::Group& S,
                                                   uint32_t& fin_tot, uint32_t& nz_tot, uint32_t& neg_tot,
                                                   uint32_t (&acc)[4], uint32_t& frozen_any, uint32_t& bad_any) {
    constexpr bool DYN = DYNM != 0;
    constexpr bool SLIP = SLIPM != 0;
    constexpr bool STAGED = DYNM == 0 || DYNM == 4 || DYNM == 5;        // action streams staged through LDS, eight steps at a time
    constexpr bool TRUSTED = DYNM == 1 || DYNM == 2;                    // both sides sampled in 0..4 by the kernel itself
    const bool sample = DYNM == 1 || DYNM == 2 || (DYNM == 3 && IO.sample_actions);
    const uint4* mix_ab = DYNM == 2 ? reinterpret_cast<const uint4*>(mix_a_in) : nullptr;   // LDS rows { a: x, y; b: z, w }
    const uint2* mix_a = DYNM == 3 ? mix_a_in : nullptr;
    const uint2* mix_b = DYNM == 3 ? mix_b_in : nullptr;
    const int8_t* pol_a = DYNM == 3 || DYNM == 4 ? pol_a_in : nullptr;
    const int8_t* pol_b = DYNM == 3 || DYNM == 5 ? pol_b_in : nullptr;
    const bool use_pol_a = DYNM == 4 || (DYNM == 3 && pol_a != nullptr), use_pol_b = DYNM == 5 || (DYNM == 3 && pol_b != nullptr);
    const bool use_mix_a = DYNM == 3 && sample && mix_a != nullptr;
    const bool use_mix_b = DYNM == 3 && sample && mix_b != nullptr;
    const bool load_a = DYNM == 0 || DYNM == 5 || (DYNM == 3 && !sample && IO.act_a != nullptr);
    const bool load_b = DYNM == 0 || DYNM == 4 || (DYNM == 3 && !sample && IO.act_b != nullptr);
    const bool lane_acc = IO.return_sum != nullptr || IO.episode_count != nullptr;
    const bool by_obs = DYNM == 2 || DYNM == 4 || DYNM == 5 || (DYNM == 3 && (use_pol_a || use_pol_b || use_mix_a || use_mix_b));
    // Action streams.  A wave's loads and stores share one completion counter and may complete out of order with
    // respect to each other, so waiting for ONE prefetched action dword means waiting for every result store issued
    // before it: with a load per step the wave drained its stores every step and sat out their write latency (the
    // step took 1.5 us of which the SIMD was busy 1.1).  Instead the action dwords of eight steps — the ticks of one
    // Philox block — are fetched a block ahead into registers, parked in the thread's sixteen private LDS dwords at
    // the block boundary (the one wait per eight steps) and read back per step by ds_read, which counts separately.
    // Plain loads, not non-temporal ones: re-read or streamed, the action rows come in faster without the hint (T = 100, 2^20
    // lanes: 7.0 - 7.3 against 6.5 - 6.9 x 10^11 env-steps/s when the 200 MB block is re-read, 6.4 against 6.35 when six blocks are
    // visited in turn; tools/labs/rollout_stream_lab.py) — unlike the single step's (step_kernel_swar, SOCCER_F_STREAM_ACTIONS).
    uint32_t aa = 0u, ab = 0u;
    uint32_t nx[16];                                                    // STAGED: the next block's action dwords, in flight
#pragma unroll
    for (int k = 0; k < 16; ++k) nx[k] = 0u;
    // issue the loads of the block whose tick-0 step is `sb` (steps outside the rollout are clamped: a harmless re-read)
    auto fetch = [&](int sb) {
        uint32_t f0 = i0; asm volatile("" : "+v"(f0));
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            int st = sb + k; st = st < 0 ? 0 : st; st = st < IO.n_steps ? st : IO.n_steps - 1;
            // The step's rows are held in scalar registers: passed through an empty asm, else the optimiser folds the row offset
            // into the per-thread address and pays a 64-bit vector multiply-add per load (16 per block of eight steps).  What
            // comes out of an asm statement is a generic pointer unless its type says global memory (flat_load otherwise).
            typedef const uint8_t __attribute__((address_space(1)))* gbytes;
            typedef const uint32_t __attribute__((address_space(1)))* gwords;
            gbytes row_a = (gbytes)(IO.act_a + (long long)st * IO.act_stride);
            gbytes row_b = (gbytes)(IO.act_b + (long long)st * IO.act_stride);
            asm volatile("" : "+s"(row_a)); asm volatile("" : "+s"(row_b));
            if (load_a) nx[2 * k] = *(gwords)(row_a + f0);
            if (load_b) nx[2 * k + 1] = *(gwords)(row_b + f0);
        }
    };
    if (STAGED) fetch(-(int)((uint32_t)tick0 & 7u));
    else {
        if (load_a) aa = *reinterpret_cast<const uint32_t*>(IO.act_a + i0);
        if (load_b) ab = *reinterpret_cast<const uint32_t*>(IO.act_b + i0);
    }
    // the observation of the current tuple (goal tuples: 0), carried along when an action depends on it
    uint32_t s_lo = 0u, s_hi = 0u;
    if (by_obs) {
        const uint32_t cc0 = swar::bfi(swar::mask_of(S.ps << 7), S.cb, S.ca);
        swar::obs4<true>(R.C, S.ra, S.ca, S.rb, S.cb, S.ps & swar::K01, swar::is_zero(cc0) | swar::is_zero(cc0 ^ R.C.Wm1x4), s_lo, s_hi);
    }
    // The byte tables of the small-pitch geometry take two dwords each and v_perm_b32 one scalar operand: the other half would
    // be moved into a vector register in front of its lookup, every step.  The steady state holds that half in a vector
    // register across the loop instead (opaque, else the optimiser sinks the move back to its use).
    swar::Consts Cv = R.C;
    if (kHoistTables<DYNM, SLIPM, GENERAL, GEO, FULL, STATS>) {
        asm volatile("" : "+v"(Cv.row_lo), "+v"(Cv.col_lo), "+v"(Cv.grow_lo), "+v"(Cv.rew_lo), "+v"(Cv.term_lo));
    }
    const swar::Consts& C = Cv;
    // the steady state carries its state in step form (swar::Carry4) from step to step
    swar::Carry4 K{};
    if (!GENERAL) K = swar::carry_of(C, S);
    const unsigned long long q = (R.lane_offset + i0) >> 2;
    uint32_t fin_loc = 0u, nz_loc = 0u, neg_loc = 0u;                   // this group's finished episodes / steps with a reward / see below
    uint32_t p0 = 0u, p1 = 0u, p2 = 0u, p3 = 0u;                        // !SLIP: the current eight-tick block, transposed
    if (!SLIP) {
        const unsigned long long bt = tick0 >> 3;
        const Philox4 b = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)bt, (uint32_t)(bt >> 32), R.key0, R.key1);
        swar::transpose4(b.w[0], b.w[1], b.w[2], b.w[3], p0, p1, p2, p3);
        for (uint32_t r = ((uint32_t)tick0 & 7u) >> 1; r != 0u; --r) { p0 = p1; p1 = p2; p2 = p3; }   // wave-uniform
    }
    for (int s = 0; s < IO.n_steps; ++s) {
        const unsigned long long tick = tick0 + (unsigned long long)s;
        const uint32_t t = (uint32_t)tick & 7u;                         // wave-uniform, like everything that steers the blocks below
        const bool new_block = t == 0u || s == 0;
        uint32_t naa = aa, nab = ab;
        if (STAGED) {
            if (new_block) {                                            // park this block's actions, fetch the next block's
#pragma unroll
                for (int k = 0; k < 16; ++k) if ((k & 1) ? load_b : load_a) act_lds[k * kBlock] = nx[k];
                if (s + 8 - (int)t < IO.n_steps) fetch(s + 8 - (int)t);
            }
            if (load_a) aa = act_lds[(2u * t) * kBlock];
            if (load_b) ab = act_lds[(2u * t + 1u) * kBlock];
        } else if (s + 1 < IO.n_steps) {                                // DYNM == 3: prefetch the next step's actions
            if (load_a) naa = *reinterpret_cast<const uint32_t*>(IO.act_a + (long long)(s + 1) * IO.act_stride + i0);
            if (load_b) nab = *reinterpret_cast<const uint32_t*>(IO.act_b + (long long)(s + 1) * IO.act_stride + i0);
        }
        uint32_t a4 = aa, b4 = ab;
        if (DYN) {
            uint32_t aw[4] = {0u, 0u, 0u, 0u};
            if (sample) {
                const Philox4 ab_blk = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)tick, (uint32_t)(tick >> 32) | 0x80000000u, R.key0, R.key1);
                aw[0] = ab_blk.w[0]; aw[1] = ab_blk.w[1]; aw[2] = ab_blk.w[2]; aw[3] = ab_blk.w[3];
                a4 = 0u; b4 = 0u;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t ob = ((j & 2 ? s_hi : s_lo) >> (16 * (j & 1))) & 0xffffu;
                if (DYNM == 2) {                    // both sides from their tables: one 16-byte LDS row per lane
                    const uint4 th = mix_ab[ob];
                    const uint32_t wm = aw[j] | 0x80008000u;
                    a4 |= count8_le15(draw_a15(wm), th.x, th.y) << (8 * j);      // 8 x the action; divided after the loop
                    b4 |= count8_le15(draw_b15(wm), th.z, th.w) << (8 * j);
                } else if (sample) {                // two actions from one 32-bit word, 15 bits each
                    const uint32_t ha = aw[j] & 0x7fffu, hb = (aw[j] >> 16) & 0x7fffu;
                    uint32_t a = (ha * 5u) >> 15, b = (hb * 5u) >> 15;          // uniform
                    const uint32_t wm = aw[j] | 0x80008000u;
                    if (use_mix_a) { const uint2 th = mix_a[ob]; a = count8_le15(draw_a15(wm), th.x, th.y) >> 3; }
                    if (use_mix_b) { const uint2 th = mix_b[ob]; b = count8_le15(draw_b15(wm), th.x, th.y) >> 3; }
                    a4 |= a << (8 * j); b4 |= b << (8 * j);
                }
                if (use_pol_a) a4 = (a4 & ~(0xffu << (8 * j))) | ((uint32_t)(uint8_t)pol_a[ob] << (8 * j));
                if (use_pol_b) b4 = (b4 & ~(0xffu << (8 * j))) | ((uint32_t)(uint8_t)pol_b[ob] << (8 * j));
            }
            if (DYNM == 2) { a4 >>= 3; b4 >>= 3; }  // every byte held 8 x (0..4): no bit crosses a byte
        }
        swar::Out o;
        uint32_t sa = 0u, sb = 0u, cls4 = 0u;
        swar::Rand4 rnd;
        if (SLIP) {
            const Philox4 blk = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)tick, (uint32_t)(tick >> 32), R.key0, R.key1);
            uint32_t k4 = 0u;
            // (the low three bits: the slip tables map 5..7 to NOOP like every other action table)
            const uint32_t ca4 = TRUSTED ? a4 : a4 & 0x07070707u, cb4 = TRUSTED ? b4 : b4 & 0x07070707u;
            if (SLIPM == 2) swar::slip_select4_lut(slip.lut, slip.T, R.L.c_off, ca4, cb4, blk.w[0], blk.w[1], blk.w[2], blk.w[3], sa, sb, k4, cls4);
            else swar::slip_select4(R.L, slip.sub, ca4, cb4, blk.w[0], blk.w[1], blk.w[2], blk.w[3], sa, sb, k4, cls4);
            rnd = swar::Rand4{k4 << 6, swar::pack_byte0(blk.w[0], blk.w[1], blk.w[2], blk.w[3]) >> C.isd_shift};
        } else {
            if (t == 0u && s != 0) {
                const unsigned long long bt = tick >> 3;
                // (the key through an empty asm: the ten round keys are then derived here, by scalar adds every eighth step, instead
                // of living in twenty scalar registers across the loop — which spilled to vector lanes and came back by v_readlane)
                uint32_t k0 = R.key0, k1 = R.key1; asm volatile("" : "+s"(k0), "+s"(k1));
                const Philox4 b = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)bt, (uint32_t)(bt >> 32), k0, k1);
                swar::transpose4(b.w[0], b.w[1], b.w[2], b.w[3], p0, p1, p2, p3);
            }
            rnd = swar::rand_pair(C.isd_shift, t, p0);
            // odd tick: the pair is used up.  The empty asm keeps this a (scalar) branch around three moves; as selects it
            // was three v_cndmask_b32 every step, each several times the cost of a move (tools/labs/valu_rate_lab.hip).
            if (t & 1u) { asm volatile(""); p0 = p1; p1 = p2; p2 = p3; }
        }
        if constexpr (GENERAL) swar::step4<true, FULL, SLIP, GEO, TRUSTED>(C, S, a4, b4, sa, sb, cls4, rnd, o);
        else swar::step4_carry<FULL, SLIP, GEO, TRUSTED>(C, K, a4, b4, sa, sb, cls4, rnd, o);
        s_lo = o.obs_lo; s_hi = o.obs_hi;
        // the step's row of every stream as a uniform base (scalar registers) + this thread's 32-bit byte offset: stores of the
        // form v_off, data, s[base] (the offset passes through an empty asm per step, else the optimiser keeps one 64-bit
        // per-thread address per stream across the loop and adds the row to it with vector instructions)
        const long long row = (long long)s * IO.out_stride;
        uint32_t j0 = i0; asm volatile("" : "+v"(j0));
        if (IO.obs) __builtin_nontemporal_store((unsigned long long)o.obs_lo | ((unsigned long long)o.obs_hi << 32),
                                                reinterpret_cast<unsigned long long*>(reinterpret_cast<uint8_t*>(IO.obs + row) + (j0 << 1)));
        if (IO.reward) __builtin_nontemporal_store(o.rew, reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(IO.reward + row) + j0));
        if (IO.terminated) __builtin_nontemporal_store(o.term, reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(IO.terminated + row) + j0));
        if (IO.truncated) __builtin_nontemporal_store(o.trunc, reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(IO.truncated + row) + j0));
        if (FULL) {     // batched_rollout_ex: what gym's vector convention reports per step next to the four streams
            if (IO.final_obs) __builtin_nontemporal_store((unsigned long long)o.fin_lo | ((unsigned long long)o.fin_hi << 32),
                                                          reinterpret_cast<unsigned long long*>(reinterpret_cast<uint8_t*>(IO.final_obs + row) + (j0 << 1)));
            if (IO.prob_code) __builtin_nontemporal_store(o.code, reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(IO.prob_code + row) + j0));
        }
        // finished episodes by return: a reward byte is 0x01 / 0xff only on the step that ends an episode
        if (STATS) fin_loc += (uint32_t)__builtin_popcount(o.finished & swar::K80);
        if (STATS && GENERAL) { nz_loc += (uint32_t)__builtin_popcount(o.rew & swar::K01); neg_loc += (uint32_t)__builtin_popcount(o.rew & swar::K80); }
        else if (STATS) {
            // without frozen / goal-tuple lanes a step terminates exactly when it carries a reward, so the clean 0 / 1 bytes of
            // `terminated` count the rewards and the bits of the reward bytes (0x01 / 0xff) count (+1) + 8 x (-1): two
            // population counts without a mask
            nz_loc += (uint32_t)__builtin_popcount(o.term); neg_loc += (uint32_t)__builtin_popcount(o.rew);
        }
        if (lane_acc) {                                             // wave-uniform
            // reward bytes sign-extended to int16 pairs (v_perm_b32's sign selectors), finished flags to 0 / 1
            acc[0] = swar::pk_add(acc[0], swar::perm(o.rew << 8, o.rew, 0x08010a00u));
            acc[1] = swar::pk_add(acc[1], swar::perm(o.rew << 8, o.rew, 0x09030b02u));
            const uint32_t f01 = swar::one_of(o.finished);
            acc[2] += swar::perm(0u, f01, 0x0c010c00u); acc[3] += swar::perm(0u, f01, 0x0c030c02u);   // <= 4096 < 2^16: no carry
        }
        if (GENERAL) frozen_any |= o.frozen;
        if (!TRUSTED) bad_any |= o.bad_action;
        if (!STAGED) { aa = naa; ab = nab; }
    }
    if (!GENERAL) S = swar::group_of(C, K);
    fin_tot += fin_loc; nz_tot += nz_loc;
    neg_tot += GENERAL ? neg_loc : (neg_loc - nz_loc) / 7u;             // (pos + 8 neg) - (pos + neg) = 7 neg
}

// FULL: also the per-step final_obs / prob_code trajectories (batched_rollout_ex; +3 B per env-step and the second observation index)
// STATS = false: the shape of a fused captured run whose handle keeps no step statistics (flush_run) — no per-step counts, no
// histogram slot is read or written (R.hist is null).  Instantiated only for the shapes such a run can take (kUnreadShape).
template <int DYNM, int SLIPM, int GEO = 0, bool FULL = false, bool STATS = true>
__global__ __launch_bounds__(kBlock) void rollout_swar_kernel(const RolloutSwar R, const RolloutIO IO) {
    constexpr bool SLIP = SLIPM != 0;
    constexpr bool DYN = DYNM >= 2;          // the forms that look something up by the observation
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    static_assert(STATS || kUnreadShape<DYNM, FULL>, "only a fused run of captured steps goes without statistics");
    HistAcc<false> hist; if (STATS) hist.init_at(R.hist, R.hist_mask);
    // LDS: the slip thresholds — SLIPM == 1: dynamic [0, 36) the nine rows; SLIPM == 2: a STATIC array (its address is an
    // immediate of the ds_read, not an add per lane) holding the bucket table and the ascending list — then, dynamic from
    // R.tab_off (DYN, when they fit), the mixed-policy rows — DYNM == 2: one 16-byte row { a's
    // four thresholds, b's four } per state; DYNM == 3: mix_a rows, then mix_b rows (8 B per state) — and the two fixed
    // policies (1 B per state), then from R.act_off the action staging area
    SlipSrc slip{R.sub, nullptr, nullptr};
    const uint2* mix_a = reinterpret_cast<const uint2*>(IO.mix_a);
    const uint2* mix_b = reinterpret_cast<const uint2*>(IO.mix_b);
    const int8_t* pol_a = DYNM == 3 || DYNM == 4 ? R.policy_a : nullptr; const int8_t* pol_b = DYNM == 3 || DYNM == 5 ? R.policy_b : nullptr;
    const bool sample = DYNM == 2 || (DYNM == 3 && IO.sample_actions);
    if (SLIP || (DYN && R.lds_tables)) {
        if (SLIPM == 1) { if (threadIdx.x < 36) smem[threadIdx.x] = reinterpret_cast<const uint32_t*>(R.sub)[threadIdx.x];
                          slip.sub = reinterpret_cast<const swar::Quad*>(smem); }
        if (SLIPM == 2) {
            __shared__ __attribute__((aligned(16))) uint32_t s_slip[SLIPM == 2 ? kSlipLutWords : 4];
            for (int i = threadIdx.x; i < kSlipLutWords; i += kBlock) s_slip[i] = R.slip_lut[i];
            slip.lut = reinterpret_cast<const uint8_t*>(s_slip); slip.T = s_slip + kSlipLutWords - 40;
        }
        if (DYNM == 2) {                     // the host picks this shape only when the rows fit
            uint4* lab = reinterpret_cast<uint4*>(smem + R.tab_off);
            for (int i = threadIdx.x; i < R.nS; i += kBlock) { const uint2 xa = mix_a[i], xb = mix_b[i]; lab[i] = make_uint4(xa.x, xa.y, xb.x, xb.y); }
            mix_a = reinterpret_cast<const uint2*>(lab); mix_b = nullptr;
        } else if (DYN && R.lds_tables) {
            uint2* la = reinterpret_cast<uint2*>(smem + R.tab_off); uint2* lb = la + R.nS;
            int8_t* pa = reinterpret_cast<int8_t*>(lb + R.nS); int8_t* pb = pa + ((R.nS + 15) & ~15);
            if (sample && mix_a) { for (int i = threadIdx.x; i < R.nS; i += kBlock) la[i] = mix_a[i]; mix_a = la; }
            if (sample && mix_b) { for (int i = threadIdx.x; i < R.nS; i += kBlock) lb[i] = mix_b[i]; mix_b = lb; }
            if (pol_a) { for (int i = threadIdx.x; i < R.nS; i += kBlock) pa[i] = pol_a[i]; pol_a = pa; }
            if (pol_b) { for (int i = threadIdx.x; i < R.nS; i += kBlock) pb[i] = pol_b[i]; pol_b = pb; }
        }
        __syncthreads();
    }
    const unsigned long long tick0 = *R.tick_in;
    if (R.tick_out && blockIdx.x == 0 && threadIdx.x == 0) *R.tick_out = tick0 + (unsigned long long)IO.n_steps;
    const unsigned long long groups = R.n >> 2;                      // the launch covers a multiple of 4 lanes
    uint32_t frozen_any = 0u, bad_any = 0u;
    uint32_t* act_lds = smem + R.act_off + threadIdx.x;              // this thread's sixteen dwords, kBlock apart
    for (unsigned long long g = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; g < groups;
         g += (unsigned long long)gridDim.x * kBlock) {
        // 32-bit byte offsets: the host hands the kernel at most kSwarLaunchLanes lanes at a time (like step_kernel_swar)
        const uint32_t i0 = (uint32_t)R.first + ((uint32_t)g << 2);
        const uint8_t* sp = R.state + i0;
        swar::Group S;
        if (R.layout == kStatePacked) {
            swar::unpack3(*reinterpret_cast<const uint32_t*>(sp), *reinterpret_cast<const uint32_t*>(sp + R.state_stride),
                          *reinterpret_cast<const uint32_t*>(sp + 2 * R.state_stride), S);
        } else {
        S.ra = *reinterpret_cast<const uint32_t*>(sp); S.ca = *reinterpret_cast<const uint32_t*>(sp + R.state_stride);
        S.rb = *reinterpret_cast<const uint32_t*>(sp + 2 * R.state_stride); S.cb = *reinterpret_cast<const uint32_t*>(sp + 3 * R.state_stride);
        S.ps = *reinterpret_cast<const uint32_t*>(sp + 4 * R.state_stride); S.tt = *reinterpret_cast<const uint32_t*>(sp + 5 * R.state_stride);
        }
        uint32_t fin_tot = 0u, nz_tot = 0u, neg_tot = 0u;
        uint32_t acc[4] = {0u, 0u, 0u, 0u};     // per lane: int16 return (two pairs), uint16 finished episodes (two pairs); T <= 4096
        // any lane frozen, any player in a goal column (= a goal tuple), or no auto-reset: the general step
        const uint32_t edge = swar::is_zero(S.ca) | swar::is_zero(S.cb) | swar::is_zero(S.ca ^ R.C.Wm1x4) | swar::is_zero(S.cb ^ R.C.Wm1x4);
        const bool special = R.C.autoreset == 0u || (((S.ps << 6) | edge) & swar::K80) != 0u;
        if (special) rollout_swar_group<DYNM, SLIPM, true, GEO, FULL, STATS>(R, IO, slip, mix_a, mix_b, pol_a, pol_b, act_lds, i0, tick0, S, fin_tot, nz_tot, neg_tot, acc, frozen_any, bad_any);
        else rollout_swar_group<DYNM, SLIPM, false, GEO, FULL, STATS>(R, IO, slip, mix_a, mix_b, pol_a, pol_b, act_lds, i0, tick0, S, fin_tot, nz_tot, neg_tot, acc, frozen_any, bad_any);
        uint8_t* sw = R.state + i0;
        if (R.layout == kStatePacked) {
            uint32_t pa, pb, pt;
            swar::pack3(S, pa, pb, pt);
            *reinterpret_cast<uint32_t*>(sw) = pa; *reinterpret_cast<uint32_t*>(sw + R.state_stride) = pb; *reinterpret_cast<uint32_t*>(sw + 2 * R.state_stride) = pt;
        } else {
        *reinterpret_cast<uint32_t*>(sw) = S.ra; *reinterpret_cast<uint32_t*>(sw + R.state_stride) = S.ca;
        *reinterpret_cast<uint32_t*>(sw + 2 * R.state_stride) = S.rb; *reinterpret_cast<uint32_t*>(sw + 3 * R.state_stride) = S.cb;
        *reinterpret_cast<uint32_t*>(sw + 4 * R.state_stride) = S.ps; *reinterpret_cast<uint32_t*>(sw + 5 * R.state_stride) = S.tt;
        }
        if (STATS) hist.add_totals(fin_tot, (int32_t)nz_tot - 2 * (int32_t)neg_tot, nz_tot);
        if (IO.return_sum != nullptr || IO.episode_count != nullptr) {
            int32_t ret[4] = {(int32_t)(int16_t)(acc[0] & 0xffffu), (int32_t)(int16_t)(acc[0] >> 16), (int32_t)(int16_t)(acc[1] & 0xffffu), (int32_t)(int16_t)(acc[1] >> 16)};
            int32_t eps[4] = {(int32_t)(acc[2] & 0xffffu), (int32_t)(acc[2] >> 16), (int32_t)(acc[3] & 0xffffu), (int32_t)(acc[3] >> 16)};
            if (IO.return_sum) add_words<4>(IO.return_sum, i0, ret);
            if (IO.episode_count) add_words<4>(IO.episode_count, i0, eps);
        }
    }
    if (frozen_any) R.misuse[0] = 1u;
    if (bad_any) R.misuse[1] = 1u;
    if (STATS) hist.flush_at(R.hist, R.hist_mask);
}

}  // namespace soccer
