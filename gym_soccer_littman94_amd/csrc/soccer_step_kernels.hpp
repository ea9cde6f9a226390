// soccer_step_kernels.hpp — the single-step kernels: step_kernel, step_kernel_hot, step_kernel_swar.
// Included by soccer_step.hip only: every kernel is emitted by exactly one translation unit.
#pragma once
#include "soccer_kernels.hpp"

namespace soccer {

// =================================================================================================
// batched_step
// =================================================================================================
// Each thread owns the 4 consecutive lanes [4g, 4g+4) and walks them in a ROLLED loop: the code of one
// lane step exists once, so a launch — which starts with a cold instruction cache — fetches ~4x less
// code than an unrolled body (measured: 12.8 -> 10.2 us per launch at 2^20 lanes).
// Bytes are peeled off the packed input dwords by shifting and results are shifted into packed output
// dwords with v_alignbyte, so no per-lane register arrays are needed.  The rule tables are read
// straight from global memory (4.3 KB, L1/L2 resident): with 3 lookups per lane a per-workgroup LDS
// staging pass + barrier costs more than it saves (measured: -0.7 us).
template <bool VEC>
__device__ __forceinline__ uint32_t load4(const void* base, unsigned long long i, int cnt) {
    const uint8_t* p = static_cast<const uint8_t*>(base) + i;
    if (VEC) return *reinterpret_cast<const uint32_t*>(p);
    uint32_t v = 0u;
    for (int k = 0; k < cnt; ++k) v |= (uint32_t)p[k] << (8 * k);
    return v;
}
template <bool VEC>
__device__ __forceinline__ void store4(void* base, unsigned long long i, int cnt, uint32_t v) {
    uint8_t* p = static_cast<uint8_t*>(base) + i;
    if (VEC) { *reinterpret_cast<uint32_t*>(p) = v; return; }
    for (int k = 0; k < cnt; ++k) p[k] = (uint8_t)(v >> (8 * k));
}
template <bool VEC>
__device__ __forceinline__ void store4h(uint16_t* base, unsigned long long i, int cnt, uint32_t lo, uint32_t hi) {
    uint16_t* p = base + i;
    if (VEC) { *reinterpret_cast<uint2*>(p) = make_uint2(lo, hi); return; }
    for (int k = 0; k < cnt; ++k) p[k] = (uint16_t)((k < 2 ? lo : hi) >> (16 * (k & 1)));
}

// VEC:    the launch covers a multiple of 4 lanes starting at a multiple of 4, all streams dword-aligned
//         (the host sends a ragged tail / misaligned buffers to the VEC = false instantiation);
// SHARED: (lane_offset + first) % 4 == 0, so a thread's 4 lanes are exactly one Philox block;
// EXPLICIT_U ("generic"): caller-supplied uniforms (u_step / u_reset) may replace the Philox draw, and
//         a fixed-policy side (single-agent mode, reference :187-188) takes its action from
//         policy[observation of the current tuple] instead of the action stream.
// This is the general kernel, with every optional output and the step statistics: it takes what the specialised
// kernels below do not — ragged tails, misaligned buffers, pitches beyond the byte arithmetic, and the exact
// float64 walk of the work list (IO.worklist).
template <bool SLIP, bool EXPLICIT_U, bool VEC, bool SHARED>
__global__ __launch_bounds__(kBlock) void step_kernel(const KernelParams P, const StepIO IO) {
    const unsigned long long groups = (P.n + 3) >> 2;
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    const unsigned long long tick = *P.tick_in;                 // scalar load; published at the end so that its miss
                                                                // does not sit in front of the first data loads
    // the episode histogram of single steps is opt-in (SOCCER_F_STEP_STATS): counting, the wave
    // reduction and the slot update cost ~0.5 us of a ~9 us launch
    const bool stats = P.step_stats != 0u;
    HistAcc<true> hist; hist.fin = 0u; hist.pos = 0u; hist.neg = 0u; hist.old01 = make_ulonglong2(0ull, 0ull); hist.old2 = 0ull;
    if (stats) hist.init(P);
    Tables T; T.lut = P.lut; T.nc = P.next_cell; T.isd = P.isd;
    bool mis = false;
    uint32_t bad_act = 0u;
    const unsigned long long todo = IO.worklist ? (unsigned long long)*IO.work_count : groups;      // (one workgroup when listed)
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < todo; k += stride) {
        const unsigned long long g = IO.worklist ? (unsigned long long)IO.worklist[k] : k;
        const unsigned long long i0 = P.first + (g << 2);
        const int cnt = VEC ? 4 : ((P.n - (g << 2)) < 4ull ? (int)(P.n - (g << 2)) : 4);
        const uint8_t* sp = P.state;
        const bool packed = P.state_layout == kStatePacked;        // wave-uniform
        uint32_t ra, ca, rb, cb, ps, tt;
        if (packed) {
            swar::Group G;
            swar::unpack3(load4<VEC>(sp, i0, cnt), load4<VEC>(sp + P.state_stride, i0, cnt), load4<VEC>(sp + 2 * P.state_stride, i0, cnt), G);
            ra = G.ra; ca = G.ca; rb = G.rb; cb = G.cb; ps = G.ps; tt = G.tt;
        } else {
            ra = load4<VEC>(sp, i0, cnt); ca = load4<VEC>(sp + P.state_stride, i0, cnt);
            rb = load4<VEC>(sp + 2 * P.state_stride, i0, cnt); cb = load4<VEC>(sp + 3 * P.state_stride, i0, cnt);
            ps = load4<VEC>(sp + 4 * P.state_stride, i0, cnt); tt = load4<VEC>(sp + 5 * P.state_stride, i0, cnt);
        }
        uint32_t aa = 0u, ab = 0u;
        if (!EXPLICIT_U || !P.policy_a) aa = load4<VEC>(IO.act_a, i0, cnt);
        if (!EXPLICIT_U || !P.policy_b) ab = load4<VEC>(IO.act_b, i0, cnt);
        // an action byte executes as table[byte & 7] with 5..7 -> NOOP, so none can index outside a rule table; any
        // byte outside 0..4 is reported (the reference raises IndexError, :393)
        { const uint32_t ca_ = swar::canon4(aa), cb_ = swar::canon4(ab); bad_act |= (ca_ ^ aa) | (cb_ ^ ab); aa = ca_; ab = cb_; }
        // randomness does not depend on the loads above: it is computed while they are in flight
        const bool need_philox = !EXPLICIT_U || (IO.u_step == nullptr) || (P.autoreset && IO.u_reset == nullptr);
        Philox4 blk{{0u, 0u, 0u, 0u}};
        if (SHARED && need_philox) blk = lane_block(P, (P.lane_offset + i0) >> 2, block_tick<SLIP>(tick), 0u);
        uint32_t nra = 0, nca = 0, nrb = 0, ncb = 0, nps = 0, ntt = 0;
        uint32_t o_rew = 0, o_term = 0, o_trunc = 0, o_code = 0, o_lo = 0, o_hi = 0, f_lo = 0, f_hi = 0, fin_mask = 0;
#pragma unroll 1
        for (int j = 0; j < cnt; ++j) {
            uint32_t w = j & 2 ? (j & 1 ? blk.w[3] : blk.w[2]) : (j & 1 ? blk.w[1] : blk.w[0]);
            if (!SHARED && need_philox) {
                const unsigned long long gl = P.lane_offset + i0 + j;
                const Philox4 b1 = lane_block(P, gl >> 2, block_tick<SLIP>(tick), 0u);
                const uint32_t sl = (uint32_t)gl & 3u;
                w = sl & 2u ? (sl & 1u ? b1.w[3] : b1.w[2]) : (sl & 1u ? b1.w[1] : b1.w[0]);
            }
            Draw d = draw_from_word<SLIP>(w, tick);
            if (EXPLICIT_U) {
                // (fetching the group's four uniforms ahead of this rolled loop was tried in round 4: slower on the slip walk,
                // 17.1 -> 20.4 us per launch at 2^20 lanes — sixteen more live registers; slip 0 takes step_kernel_swar<.., EXPL>)
                if (IO.u_step) { const double raw = IO.u_step[i0 + j]; const double u = sane_uniform(raw); d.u = SLIP ? sane_uniform_walk(raw) : u; d.top2 = (uint32_t)(u * 4.0); }
                if (IO.u_reset) d.reset2 = (uint32_t)(sane_uniform(IO.u_reset[i0 + j]) * 4.0);
            }
            // byte j of every packed stream: one v_bfe_u32 each (the offset 8*j is wave-uniform)
            const uint32_t sh = 8u * (uint32_t)j;
            const uint32_t psj = __builtin_amdgcn_ubfe(ps, sh, 8u);
            Lane L;
            L.A = make_pos(__builtin_amdgcn_ubfe(ra, sh, 8u), __builtin_amdgcn_ubfe(ca, sh, 8u), P.W);
            L.B = make_pos(__builtin_amdgcn_ubfe(rb, sh, 8u), __builtin_amdgcn_ubfe(cb, sh, 8u), P.W);
            L.p = psj & 1u; L.need = (psj >> 1) & 1u; L.t = __builtin_amdgcn_ubfe(tt, sh, 8u);
            uint32_t a_now = __builtin_amdgcn_ubfe(aa, sh, 8u), b_now = __builtin_amdgcn_ubfe(ab, sh, 8u);
            if (EXPLICIT_U && (P.policy_a || P.policy_b)) {         // the fixed side acts on the current observation
                const uint32_t s_now = obs_of(T, P, L.A, L.B, L.p);
                if (P.policy_a) a_now = (uint32_t)(uint8_t)P.policy_a[s_now];
                if (P.policy_b) b_now = (uint32_t)(uint8_t)P.policy_b[s_now];
            }
            StepResult R;
            // a caller-supplied uniform is an arbitrary double; without one the draw is the lane's Philox word
            // (fixed-policy handles take this kernel too) and the integer slip decision applies
            if (EXPLICIT_U && IO.u_step) mis |= lane_step<SLIP, false>(T, P, L, a_now, b_now, d, R);
            else mis |= lane_step<SLIP, true>(T, P, L, a_now, b_now, d, R);
            nra = __builtin_amdgcn_alignbyte(L.A >> 24, nra, 1); nca = __builtin_amdgcn_alignbyte((L.A >> 16) & 0xffu, nca, 1);
            nrb = __builtin_amdgcn_alignbyte(L.B >> 24, nrb, 1); ncb = __builtin_amdgcn_alignbyte((L.B >> 16) & 0xffu, ncb, 1);
            nps = __builtin_amdgcn_alignbyte(L.p | (L.need << 1), nps, 1); ntt = __builtin_amdgcn_alignbyte(L.t, ntt, 1);
            o_rew = __builtin_amdgcn_alignbyte((uint32_t)R.reward & 0xffu, o_rew, 1);
            o_term = __builtin_amdgcn_alignbyte(R.term, o_term, 1); o_trunc = __builtin_amdgcn_alignbyte(R.trunc, o_trunc, 1);
            o_code = __builtin_amdgcn_alignbyte(R.code, o_code, 1);
            o_lo = __builtin_amdgcn_alignbit(o_hi, o_lo, 16); o_hi = (o_hi >> 16) | (R.obs << 16);
            f_lo = __builtin_amdgcn_alignbit(f_hi, f_lo, 16); f_hi = (f_hi >> 16) | (R.final_obs << 16);
            fin_mask |= R.finished << j;
            if (stats) hist.add(R.finished, R.reward);
        }
        if (!VEC && cnt < 4) {               // ragged tail: the shifted-in bytes sit at the top
            const int sh = 8 * (4 - cnt);
            nra >>= sh; nca >>= sh; nrb >>= sh; ncb >>= sh; nps >>= sh; ntt >>= sh;
            o_rew >>= sh; o_term >>= sh; o_trunc >>= sh; o_code >>= sh;
            for (int k = cnt; k < 4; ++k) {
                o_lo = __builtin_amdgcn_alignbit(o_hi, o_lo, 16); o_hi >>= 16;
                f_lo = __builtin_amdgcn_alignbit(f_hi, f_lo, 16); f_hi >>= 16;
            }
        }
        uint8_t* sw = P.state;
        if (packed) {
            uint32_t pa, pb, pt;
            swar::pack3(swar::Group{nra, nca, nrb, ncb, nps, ntt}, pa, pb, pt);
            store4<VEC>(sw, i0, cnt, pa); store4<VEC>(sw + P.state_stride, i0, cnt, pb); store4<VEC>(sw + 2 * P.state_stride, i0, cnt, pt);
        } else {
            store4<VEC>(sw, i0, cnt, nra); store4<VEC>(sw + P.state_stride, i0, cnt, nca);
            store4<VEC>(sw + 2 * P.state_stride, i0, cnt, nrb); store4<VEC>(sw + 3 * P.state_stride, i0, cnt, ncb);
            store4<VEC>(sw + 4 * P.state_stride, i0, cnt, nps); store4<VEC>(sw + 5 * P.state_stride, i0, cnt, ntt);
        }
        if (IO.obs) store4h<VEC>(IO.obs, i0, cnt, o_lo, o_hi);
        if (IO.reward) store4<VEC>(IO.reward, i0, cnt, o_rew);
        if (IO.terminated) store4<VEC>(IO.terminated, i0, cnt, o_term);
        if (IO.truncated) store4<VEC>(IO.truncated, i0, cnt, o_trunc);
        if (IO.prob_code) store4<VEC>(IO.prob_code, i0, cnt, o_code);
        if (IO.final_obs) store4h<VEC>(IO.final_obs, i0, cnt, f_lo, f_hi);
        if (IO.last_return && fin_mask) {
            for (int j = 0; j < cnt; ++j)
                if ((fin_mask >> j) & 1u) IO.last_return[i0 + j] = (int8_t)(o_rew >> (8 * j));
        }
        if (IO.reward_a_f32 || IO.reward_b_f32 || IO.finished) {
            for (int j = 0; j < cnt; ++j) {
                const float f = (float)(int8_t)(o_rew >> (8 * j));
                if (IO.reward_a_f32) IO.reward_a_f32[i0 + j] = f;
                if (IO.reward_b_f32) IO.reward_b_f32[i0 + j] = 0.0f - f;
                if (IO.finished) IO.finished[i0 + j] = (uint8_t)(((o_term | o_trunc) >> (8 * j)) & 1u);
            }
        }
    }
    if (mis) P.misuse[0] = 1u;
    if (bad_act) P.misuse[1] = 1u;
    if (stats) hist.flush(P);
    if (P.tick_out) publish_tick(P, tick, 1ull);
    if (IO.worklist) {                       // launched as ONE workgroup: everyone has read the count, the list is consumed
        __syncthreads();
        if (threadIdx.x == 0) {
            *IO.work_count = 0u;
            // the statistics behind the count (8-byte aligned, soccer_exact_walk_stats): launch parts, groups walked
            unsigned long long* st = reinterpret_cast<unsigned long long*>(IO.work_count + 2);
            st[0] += 1ull; st[1] += todo;
        }
    }
}

// The instantiation every Philox-driven, dword-aligned, 4-outputs-only step takes (bench.py's path):
// one group of 4 lanes per thread, no grid-stride loop, no fallback or optional-output code at all.
// Same lane loop as step_kernel; kept separate because a launch starts with a cold instruction cache
// and every instruction that is not fetched counts (-0.4 us per launch against a step_kernel instantiation with the optional outputs compiled out).
template <bool SLIP, bool INT_ONLY = false>
__device__ __forceinline__ void hot_group(const KernelParams& P, const StepIO& IO, unsigned long long g,
                                          const unsigned long long* tick_ptr, unsigned long long tick_val) {
    const unsigned long long i0 = P.first + (g << 2);
    Tables T; T.lut = P.lut; T.nc = P.next_cell; T.isd = P.isd;
    const uint8_t* sp = P.state;
#define SOCCER_LD(p) __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p))
    const bool packed = P.state_layout == kStatePacked;            // wave-uniform
    uint32_t ra, ca, rb, cb, ps, tt;
    if (packed) {
        const uint32_t pa = SOCCER_LD(sp + i0), pb = SOCCER_LD(sp + P.state_stride + i0);
        tt = SOCCER_LD(sp + 2 * P.state_stride + i0);
        ra = pa; ca = pb; rb = 0u; cb = 0u; ps = 0u;                // taken apart below, behind the action loads
    } else {
        ra = SOCCER_LD(sp + i0);
        ca = SOCCER_LD(sp + P.state_stride + i0);
        rb = SOCCER_LD(sp + 2 * P.state_stride + i0);
        cb = SOCCER_LD(sp + 3 * P.state_stride + i0);
        ps = SOCCER_LD(sp + 4 * P.state_stride + i0);
        tt = SOCCER_LD(sp + 5 * P.state_stride + i0);
    }
    uint32_t aa = SOCCER_LD(IO.act_a + i0), ab = SOCCER_LD(IO.act_b + i0);
    if (packed) { swar::Group G; swar::unpack3(ra, ca, tt, G); ra = G.ra; ca = G.ca; rb = G.rb; cb = G.cb; ps = G.ps; }
#undef SOCCER_LD
    // action bytes execute as table[byte & 7] with 5..7 -> NOOP; anything outside 0..4 is reported (:393)
    const uint32_t aa_raw = aa, ab_raw = ab;
    aa = swar::canon4(aa); ab = swar::canon4(ab);
    // The tick comes from device memory (graph replays cannot change kernel arguments).  It is read AFTER the
    // eight data loads above have been issued: read first, its scalar-cache miss (~1 us) sat in front of them.
    const unsigned long long tick = tick_ptr ? *tick_ptr : tick_val;
    if (P.tick_out) publish_tick(P, tick, 1ull);
    // the thread's 4 lanes are exactly one Philox block; computed while the loads are in flight
    const Philox4 blk = lane_block(P, (P.lane_offset + i0) >> 2, block_tick<SLIP>(tick), 0u);
    uint32_t nra = 0, nca = 0, nrb = 0, ncb = 0, nps = 0, ntt = 0, o_rew = 0, o_term = 0, o_trunc = 0, o_lo = 0, o_hi = 0;
    uint32_t posA[4] = {0u, 0u, 0u, 0u}, posB[4] = {0u, 0u, 0u, 0u};
    bool mis = false;
#pragma unroll 4
    for (int j = 0; j < 4; ++j) {
        const uint32_t w = j & 2 ? (j & 1 ? blk.w[3] : blk.w[2]) : (j & 1 ? blk.w[1] : blk.w[0]);
        const uint32_t sh = 8u * (uint32_t)j;
        const uint32_t psj = __builtin_amdgcn_ubfe(ps, sh, 8u);
        Lane L;
        L.A = make_pos(__builtin_amdgcn_ubfe(ra, sh, 8u), __builtin_amdgcn_ubfe(ca, sh, 8u), P.W);
        L.B = make_pos(__builtin_amdgcn_ubfe(rb, sh, 8u), __builtin_amdgcn_ubfe(cb, sh, 8u), P.W);
        L.p = psj & 1u; L.need = (psj >> 1) & 1u; L.t = __builtin_amdgcn_ubfe(tt, sh, 8u);
        StepResult R;
        const uint32_t a_now = __builtin_amdgcn_ubfe(aa, sh, 8u), b_now = __builtin_amdgcn_ubfe(ab, sh, 8u);
        mis |= lane_step<SLIP, true, INT_ONLY>(T, P, L, a_now, b_now, draw_from_word<SLIP>(w, tick), R);
        posA[j] = L.A; posB[j] = L.B;                                   // rows / columns gathered with v_perm after the loop
        nps = __builtin_amdgcn_alignbyte(L.p | (L.need << 1), nps, 1); ntt = __builtin_amdgcn_alignbyte(L.t, ntt, 1);
        o_rew = __builtin_amdgcn_alignbyte((uint32_t)R.reward & 0xffu, o_rew, 1);
        o_term = __builtin_amdgcn_alignbyte(R.term, o_term, 1); o_trunc = __builtin_amdgcn_alignbyte(R.trunc, o_trunc, 1);
        o_lo = __builtin_amdgcn_alignbit(o_hi, o_lo, 16); o_hi = (o_hi >> 16) | (R.obs << 16);
    }
    // the row (byte 3) and column (byte 2) of four position words -> the packed row / column dwords: 4 byte
    // permutes per player instead of a shift + funnel shift per lane and field (v_perm_b32 picks bytes 0-3 from
    // its second operand, 4-7 from its first)
    const uint32_t a01 = __builtin_amdgcn_perm(posA[1], posA[0], 0x07030602u), a23 = __builtin_amdgcn_perm(posA[3], posA[2], 0x07030602u);
    const uint32_t b01 = __builtin_amdgcn_perm(posB[1], posB[0], 0x07030602u), b23 = __builtin_amdgcn_perm(posB[3], posB[2], 0x07030602u);
    nca = __builtin_amdgcn_perm(a23, a01, 0x05040100u); nra = __builtin_amdgcn_perm(a23, a01, 0x07060302u);
    ncb = __builtin_amdgcn_perm(b23, b01, 0x05040100u); nrb = __builtin_amdgcn_perm(b23, b01, 0x07060302u);
    uint8_t* sw = P.state;
    // the state is re-read by the NEXT launch only, i.e. after the kernel-boundary write-back / invalidate of L2:
    // streaming it as well is worth another ~1 % (6.91 -> 6.83 us)
#define SOCCER_ST(p, v) __builtin_nontemporal_store((v), reinterpret_cast<uint32_t*>(p))
    if (packed) {
        uint32_t pa, pb, pt;
        swar::pack3(swar::Group{nra, nca, nrb, ncb, nps, ntt}, pa, pb, pt);
        SOCCER_ST(sw + i0, pa); SOCCER_ST(sw + P.state_stride + i0, pb); SOCCER_ST(sw + 2 * P.state_stride + i0, pt);
    } else {
        SOCCER_ST(sw + i0, nra); SOCCER_ST(sw + P.state_stride + i0, nca);
        SOCCER_ST(sw + 2 * P.state_stride + i0, nrb); SOCCER_ST(sw + 3 * P.state_stride + i0, ncb);
        SOCCER_ST(sw + 4 * P.state_stride + i0, nps); SOCCER_ST(sw + 5 * P.state_stride + i0, ntt);
    }
    // Results are written once and never re-read by these kernels, actions are read once: non-temporal accesses
    // keep them from displacing the resident state in L2 / Infinity Cache (7.66 -> 6.97 us per launch).
    if (IO.obs) __builtin_nontemporal_store((unsigned long long)o_lo | ((unsigned long long)o_hi << 32),
                                            reinterpret_cast<unsigned long long*>(IO.obs + i0));
    if (IO.reward) SOCCER_ST(IO.reward + i0, o_rew);
    if (IO.terminated) SOCCER_ST(IO.terminated + i0, o_term);
    if (IO.truncated) SOCCER_ST(IO.truncated + i0, o_trunc);
#undef SOCCER_ST
    if (mis) P.misuse[0] = 1u;
    if ((aa ^ aa_raw) | (ab ^ ab_raw)) P.misuse[1] = 1u;
}

// The seven leading scalar arguments (14 dwords) repeat the fields of P / IO that the first loads depend on
// (the hot path always starts at lane 0 of the handle):
// the library is built with -mllvm -amdgpu-kernarg-preload-count=14, so they arrive in SGPRs at wave launch
// and the data loads can be issued without first waiting for a scalar load of the kernarg segment — as long as nothing
// else the addresses or the branches ahead of the loads need lives in P / IO: whatever does is one scalar-memory round trip
// in front of the first load again.  (Measured when it was introduced: -0.16 us per launch; the floor lab's copy kernel
// does not see such a round trip at all, profiles/kernarg_floor.md.)  The rest of P is fetched while the loads are in flight.
template <bool SLIP, bool INT_ONLY = false>
__global__ __launch_bounds__(kBlock) void step_kernel_hot(uint8_t* state, unsigned long long state_stride,
                                                          const int8_t* act_a, const int8_t* act_b,
                                                          const unsigned long long* tick_in,
                                                          unsigned long long n, unsigned long long tick_val,
                                                          const KernelParams P, const StepIO IO) {
    // tick_in == nullptr: an eager launch — the host knows the tick and passes it by value (tick_val), which takes the
    // scalar load off the path (-2.4 %); captured launches read the device slot (their arguments are frozen).
    const unsigned long long g = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if ((g << 2) >= n) return;                                      // n is a multiple of 4 here; the first lane is 0
    KernelParams Q = P; Q.state = state; Q.state_stride = state_stride; Q.n = n; Q.first = 0ull;
    StepIO J = IO; J.act_a = act_a; J.act_b = act_b;
    hot_group<SLIP, INT_ONLY>(Q, J, g, tick_in, tick_val);
}

// =================================================================================================
// batched_step, byte-parallel: the four lanes of a thread stay packed in their dwords (soccer_swar.hpp)
// =================================================================================================
// Same launch shape and memory behaviour as step_kernel_hot (one 4-lane group per thread, non-temporal dword
// loads — five with the packed state, eight with six streams —, the Philox block computed while they are in
// flight, seven or ten non-temporal stores, leading scalar
// arguments preloaded into SGPRs) — but no byte peeling, no per-lane loop and NO rule-table read: ~45 vector
// instructions per env-step instead of ~128 and no dependent gather between the loads and the stores.
// What is fetched when (profiles/kernarg_ab.md):
//   preloaded (14 dwords)   the state base and stride, the two action bases, tick_in, the lane count with the action-load policy
//                           in its bit 0, tick_val: all the addresses of the data loads and the branch ahead of the action loads
//                           need — no scalar memory load stands between wave start and the data loads (SLIPM == 2 fetches the
//                           pointer of its table, the one thing its table loads need beyond that);
//   one batch of s_loads    everything else the launch reads of SwarParams (constants, keys, lane_offset, the result pointers,
//                           tick_out, misuse), issued around the data loads and waited for ONCE, together with the tick,
//                           ahead of the Philox block;
//   nothing                 between the arithmetic and the stores.
// Takes every Philox-driven, dword-aligned step of a slip_prob == 0 handle whose pitch fits the byte arithmetic
// (swar::fits: every golden pitch up to 11x7 does); the template parameters are described above the kernel.
// What the OUT = 0 shape reads comes first and contiguous, so that the one batch of scalar loads the kernel issues behind its
// data loads touches as few cache lines of the argument block as possible; what only other shapes read goes behind.  (No
// `first`: the host offsets every pointer itself, the kernel's lane 0 is the launch part's first lane.  The action-load
// policy rides in bit 0 of the preloaded lane count.)
struct SwarParams {
    swar::Consts C;
    uint32_t key0, key1;
    unsigned long long lane_offset;         // global lane of the launch part's lane 0; multiple of 4
    unsigned long long* tick_out;
    unsigned int* misuse;                   // [0] a frozen lane was stepped (:376), [1] an action byte outside 0..4 (:393)
    uint16_t* obs; int8_t* reward; uint8_t* terminated; uint8_t* truncated;
    // ---- other shapes only ----
    float* reward_a_f32; float* reward_b_f32; uint8_t* finished; int8_t* last_return;   // OUT >= 1
    uint8_t* prob_code; uint16_t* final_obs;                          // OUT == 2
    unsigned long long* hist; uint32_t hist_mask;   // OUT == 2: episode histogram slots (SOCCER_F_STEP_STATS), or nullptr
    swar::SlipConsts L; const swar::Quad* sub;   // SLIPM == 1: integer cumulative weights / the nine rows of quarter thresholds
    const uint32_t* slip_lut;               // SLIPM == 2: SlipTables::lut_step (kSlipStepBuckets bytes), then T (kSlipThresholds words)
    const int8_t* policy_a; const int8_t* policy_b;   // POLICY: the fixed side's int8[nS] policy (the other is nullptr)
    const double* u_step; const double* u_reset;   // EXPL: caller-supplied uniforms (16-byte aligned; either may be nullptr: Philox then)
    const SlipF64* f64;                            // SLIPM == 3: the nominal float64 thresholds of the slip list
    uint32_t* worklist; uint32_t* work_count;      // SLIPM == 3: groups left to the exact walk (see StepIO)
};


// OUT — which outputs the instantiation can write (every pointer may still be NULL):
//   0  obs / reward / terminated / truncated: the 8-argument batched_step (19 B per env-step)
//   1  + reward_a_f32 / reward_b_f32 / finished / last_return: what a gym-style loop reads every step, without the `info`
//      extras (VectorSoccerEnv(io="device", info=False): 27 B per env-step when the int8 reward stream is left out)
//   2  + final_obs / prob_code and, when Q.hist is set, the episode histogram (VectorSoccerEnv's info; 31 B)
// Launch shape (tools/labs/swar_sweep.sh, profiles/r02_sweep.md): one 4-lane group per thread with non-temporal dword
// accesses measured best; 8 or 16 lanes per thread (dwordx2 / dwordx4), plain or write-through stores and 512-thread
// workgroups were all equal or slower, and an instantiation without the frozen-lane / goal-tuple code was not faster
// (the kernel is bound by launch + memory latency, not by vector issue any more).
// SLIPM: handles with slip_prob > 0 whose integer slip decision is the reference's for every draw (SlipTables::swar_ok).
//   1  each lane counts the integer cumulative weights and its combination's quarter points below its draw, one by one (the
//      threshold rows are gathered while the state loads are still in flight: they depend on the random word only) — ~30 vector
//      instructions per lane;
//   2  (SlipTables::lut_step_ok: slips within about [0.09, 0.96]) by table, like the rollout: a launch lives for one step, so
//      each WAVE stages what one 16-byte load per lane brings in — 1 024 byte buckets over the draw's top 10 bits — and the
//      threshold list (one entry per lane), issued ahead of the state loads and parked in the wave's own 1 280 bytes of LDS while those
//      are in flight (no workgroup barrier); a lane then needs two LDS reads and two exact compares (~9 instructions).  The table cannot be gathered from global memory instead: a wave's
//      loads return in order, so a gather issued after the state loads waits for all of them, and the 16 KB table of the
//      rollout is two dependent L2 round trips on top (5.15 us per launch, the same as comparing one by one; a 64 KB table with
//      the candidate inlined, one gather, thrashes the 16 KB L1: 6.05 us).
// Without SLIP the thread's block is the one of tick >> 3 and the lanes' draws are this tick's nibbles (swar::rand_nibble).
// POLICY: single-agent handles — the fixed side's action is looked up from its int8[nS] policy by the observation of
// the CURRENT tuple (four byte gathers per thread, behind the state loads); that side's action stream may be NULL.
// EXPL (slip_prob == 0 handles): the caller's own uniforms (batched_step_ex's u_step / u_reset: the reference-RNG replay path,
// e.g. a host that keeps the reference's MT19937 streams) replace the lanes' Philox bits.  Every list probability is 1, 1/2
// or 1/4 and the ISD is uniform over 4 or 2 entries, so floor(4u) IS the reference's first-exceeds decision for any double
// (:395, :414; values outside [0, 1) and NaN select index 0 like argmax of an all-False array): four doubles per stream and
// thread, two 16-byte loads each, issued with the state loads; round 3 sent these calls to the per-lane kernel (11.0 us).
// LAYOUT (StateLayout): three packed state streams (5 loads + 7 stores, 13 B per env-step) or six (8 + 10, 19 B) — a compile-time
// shape because a uniform branch ahead of the loads costs the SGPR-base addressing (see the action loads).
template <int OUT, int SLIPM = 0, bool POLICY = false, int GEO = 0, bool EXPL = false, uint32_t LAYOUT = kStatePacked>
__global__ __launch_bounds__(kBlock) void step_kernel_swar(const uint8_t* state_in, unsigned long long state_stride,
                                                           const int8_t* act_a, const int8_t* act_b,
                                                           const unsigned long long* tick_in,
                                                           unsigned long long n_policy, unsigned long long tick_val,
                                                           const SwarParams Q) {
    constexpr bool FULL = OUT == 2;
    constexpr bool SLIP = SLIPM != 0;
    static_assert((SLIPM == 3) ? EXPL : (!EXPL || SLIPM == 0), "caller-supplied uniforms: SLIPM 0 (dyadic lists) or 3 (float64 slip decision)");
    static_assert(kSlipStepBuckets == 64 * 16 && kSlipThresholds <= 64, "one 16-byte piece of the table per lane of a wave");
    const unsigned long long g = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    // the lane count is a multiple of 4 here; its bit 0 is the action-load policy (SOCCER_F_STREAM_ACTIONS), which the branch
    // ahead of the action loads needs: all 14 preloaded dwords are taken, and a policy fetched from the argument block would put
    // a scalar-memory round trip in front of the first data load
    const unsigned long long n = n_policy & ~3ull;
    const bool act_stream = ((uint32_t)n_policy & 1u) != 0u;
    const bool active = (g << 2) < n;
    // SLIPM == 2: this lane's 16 bytes of the bucket table and its entry of the threshold list — the oldest loads
    // of the wave, so the wait for them does not wait for the state.  Every WAVE keeps a copy of its own: no workgroup barrier.
    const uint32_t lane = threadIdx.x & 63u;
    uint4 st_lut = make_uint4(0u, 0u, 0u, 0u); uint32_t st_thr = 0u;
    if (SLIPM == 2) {
        st_lut = reinterpret_cast<const uint4*>(Q.slip_lut)[lane];
        st_thr = Q.slip_lut[kSlipStepBuckets / 4 + lane];                 // (the list is padded to 64 entries)
    }
    if (SLIPM != 2 && !FULL && !active) return;
    HistAcc<true> hist;
    if (FULL) { hist.fin = 0u; hist.pos = 0u; hist.neg = 0u; hist.old01 = make_ulonglong2(0ull, 0ull); hist.old2 = 0ull; }
    // Byte offsets are 32-bit (the host launches at most kSwarLaunchLanes lanes at a time): a uniform base plus a 32-bit
    // per-thread offset is what the compiler turns into SGPR-base addressing (global_load v, v_off, s[base:base+1]) — no
    // 64-bit vector add per stream (20 vector instructions of about 245 with 64-bit offsets).
    // The offset is made of the thread's index alone, and the bases are preloaded: NOTHING is fetched from the argument block
    // between wave start and the data loads.
    const uint32_t i0 = (uint32_t)g << 2;
#define AT(base, off) (reinterpret_cast<const uint8_t*>(base) + (off))
    const uint8_t* sp = state_in;
    swar::Group S{0u, 0u, 0u, 0u, 0u, 0u};
    uint32_t aa = 0u, ab = 0u;
    // SLIPM == 2: the state loads are issued by every lane (lanes beyond n re-read the first group) — under a branch the wait for
    // the table loads ahead of them could no longer count on their order and would become a wait for everything
    const bool fetch = SLIPM == 2 ? true : active;
    const uint32_t l0 = SLIPM == 2 ? (active ? i0 : 0u) : i0;
    if (fetch) {
        // The action streams first, by plain loads unless the caller asked for the non-temporal hint (include/soccer_hip.h): buffers
        // written or read a few steps ago are served from the Infinity Cache, and a non-temporal load gives that up — 0.2 us per
        // launch at 2^20 lanes — while action data streaming in from HBM is 0.4 us per launch faster with the hint (DESIGN.md
        // 4.3).  Both arms issue the same number of loads, so the waits below still count on the order.
        const bool ld_a = !POLICY || !Q.policy_a, ld_b = !POLICY || !Q.policy_b;
        // (each block gets the offset through an empty asm of its own: instruction selection works a block at a time and only
        // turns base + offset into SGPR-base addressing when it sees the addition in the block of the access)
        if (act_stream) {
            uint32_t la = l0; asm("" : "+v"(la));
            if (ld_a) aa = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(AT(act_a, la)));
            if (ld_b) ab = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(AT(act_b, la)));
        } else {
            // (written as wavefront-scope relaxed atomic loads — plain global_load_dword instructions — because the optimiser
            // merges two arms that differ in nothing but the non-temporal hint, and drops the hint)
            uint32_t la = l0; asm("" : "+v"(la));
            if (ld_a) aa = __hip_atomic_load(reinterpret_cast<const uint32_t*>(AT(act_a, la)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            if (ld_b) ab = __hip_atomic_load(reinterpret_cast<const uint32_t*>(AT(act_b, la)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
        uint32_t ls = l0; asm("" : "+v"(ls));
        if (LAYOUT == kStatePacked) {
            // (held in ra / ca until the step needs them: swar::unpack3 below, behind everything that does not depend on the state)
            S.ra = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(AT(sp, ls)));
            S.ca = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(AT(sp + state_stride, ls)));
            S.tt = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(AT(sp + 2 * state_stride, ls)));
        } else {
            S.ra = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(AT(sp, ls)));
            S.ca = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(AT(sp + state_stride, ls)));
            S.rb = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(AT(sp + 2 * state_stride, ls)));
            S.cb = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(AT(sp + 3 * state_stride, ls)));
            S.ps = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(AT(sp + 4 * state_stride, ls)));
            S.tt = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(AT(sp + 5 * state_stride, ls)));
        }
    }
    // the tick: by value for eager launches, from the device slot for captured ones (read after the data loads are issued)
    const unsigned long long tick = tick_in ? *tick_in : tick_val;
    // Everything else the launch needs of the argument block is requested HERE, in one batch right behind the data loads and
    // beside the tick: the pointers the stores need and the constants that only the step reads — which the compiler would
    // otherwise fetch where they are used, one scalar-memory round trip after the other between the arithmetic and the
    // stores — are inputs of an empty statement whose output is the Philox key, so they are in registers before the Philox
    // block starts.  Scalar loads return out of order: the one wait ahead of the Philox block, which the tick needs anyway,
    // covers the batch.  (The pointers are inputs only, so they keep their address space; the statement is not `volatile`: a
    // volatile asm counts as a write to memory, and scalar loads behind it would become vector loads.)
    // (not with SLIPM == 3: those shapes hold the float64 thresholds in scalar registers across the comparisons, and another
    // dozen live pointers there end in scratch memory; their stores fetch their pointers where they are used, as before)
    constexpr bool PIN = SLIPM != 3;
    uint32_t key0 = Q.key0;
    unsigned long long* const tick_out = Q.tick_out; unsigned int* const misuse = Q.misuse;
    uint16_t* const o_obs = Q.obs; int8_t* const o_reward = Q.reward; uint8_t* const o_term = Q.terminated; uint8_t* const o_trunc = Q.truncated;
    if (PIN) asm("" : "+s"(key0) : "s"(tick_out), "s"(misuse), "s"(o_obs), "s"(o_reward), "s"(o_term), "s"(o_trunc),
                                   "s"(Q.C.Wx2), "s"(Q.C.Wm2x2), "s"(Q.C.Wm1x4), "s"(Q.C.trunc_add), "s"(Q.C.obs_mul));
    float* const o_raf = OUT >= 1 ? Q.reward_a_f32 : nullptr; float* const o_rbf = OUT >= 1 ? Q.reward_b_f32 : nullptr;
    uint8_t* const o_fin = OUT >= 1 ? Q.finished : nullptr; int8_t* const o_last = OUT >= 1 ? Q.last_return : nullptr;
    if (PIN && OUT >= 1) asm("" : "+s"(key0) : "s"(o_raf), "s"(o_rbf), "s"(o_fin), "s"(o_last));
    uint8_t* const o_code = FULL ? Q.prob_code : nullptr; uint16_t* const o_fobs = FULL ? Q.final_obs : nullptr;
    unsigned long long* const hist_at = FULL ? Q.hist : nullptr; const uint32_t hist_mask = FULL ? Q.hist_mask : 0u;
    if (PIN && FULL) asm("" : "+s"(key0) : "s"(o_code), "s"(o_fobs), "s"(hist_at), "s"(hist_mask));
    // (the wave's histogram slot is read behind the data loads as well: its address comes from the argument block)
    const bool stats = FULL && hist_at != nullptr;                   // wave-uniform
    if (stats) hist.init_at(hist_at, hist_mask);
    // EXPL: the four lanes' uniforms, as floor(4u) (two bits each) — behind the state loads, ahead of the Philox block
    uint32_t xq = 0u, xr = 0u;
    double us0 = 0.0, us1 = 0.0, us2 = 0.0, us3 = 0.0;               // SLIPM == 3: the step uniforms themselves
    if (SLIPM == 3 && active) {
        const double2 a = *reinterpret_cast<const double2*>(Q.u_step + i0), b = *reinterpret_cast<const double2*>(Q.u_step + i0 + 2);
        us0 = a.x; us1 = a.y; us2 = b.x; us3 = b.y;
    }
    if (EXPL && active) {
        auto quarters = [&](const double* base) {
            const double2 a = *reinterpret_cast<const double2*>(base + i0), b = *reinterpret_cast<const double2*>(base + i0 + 2);
            return (uint32_t)(sane_uniform(a.x) * 4.0) | ((uint32_t)(sane_uniform(a.y) * 4.0) << 8) |
                   ((uint32_t)(sane_uniform(b.x) * 4.0) << 16) | ((uint32_t)(sane_uniform(b.y) * 4.0) << 24);
        };
        if (SLIPM != 3 && Q.u_step) xq = quarters(Q.u_step);
        if (Q.u_reset) xr = quarters(Q.u_reset);
    }
    const unsigned long long q = (Q.lane_offset + i0) >> 2;     // the thread's 4 lanes are exactly one Philox block
    const unsigned long long bt = block_tick<SLIP>(tick);
    Philox4 blk{{0u, 0u, 0u, 0u}};
    if (!EXPL || !Q.u_step || !Q.u_reset)                           // (wave-uniform; both uniforms supplied: no block is needed)
        blk = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)bt, (uint32_t)(bt >> 32), key0, Q.key1);
    const uint8_t* slip_lut = nullptr; const uint32_t* slip_thr = nullptr;
    if (SLIPM == 2) {                                                // park the table: all 64 lanes, whether their lanes exist or not
        __shared__ __attribute__((aligned(16))) uint32_t s_slip[SLIPM == 2 ? kBlock / 64 : 1][SLIPM == 2 ? kSlipStepLdsWords : 4];
        uint32_t* mine = s_slip[threadIdx.x >> 6];
        reinterpret_cast<uint4*>(mine)[lane] = st_lut;
        mine[kSlipStepBuckets / 4 + lane] = st_thr;
        // a wave's LDS operations complete in order; the fences keep the compiler from moving the reads below above the writes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        slip_lut = reinterpret_cast<const uint8_t*>(mine); slip_thr = mine + kSlipStepBuckets / 4;
        if (!FULL && !active) return;
    }
    if (active) {
        // (without a fixed policy nothing ahead of the step reads the state: it is taken apart behind step4_moves, below)
        if (LAYOUT == kStatePacked && POLICY) swar::unpack3(S.ra, S.ca, S.tt, S);
        if (POLICY) {                                               // the fixed side acts on the current observation (:187-188)
            uint32_t s_lo, s_hi;
            const uint32_t cc0 = swar::bfi(swar::mask_of(S.ps << 7), S.cb, S.ca);
            swar::obs4<true>(Q.C, S.ra, S.ca, S.rb, S.cb, S.ps & swar::K01, swar::is_zero(cc0) | swar::is_zero(cc0 ^ Q.C.Wm1x4), s_lo, s_hi);
            const int8_t* pol = Q.policy_a ? Q.policy_a : Q.policy_b;
            const uint32_t act = (uint32_t)(uint8_t)pol[s_lo & 0xffffu] | ((uint32_t)(uint8_t)pol[s_lo >> 16] << 8) |
                                 ((uint32_t)(uint8_t)pol[s_hi & 0xffffu] << 16) | ((uint32_t)(uint8_t)pol[s_hi >> 16] << 24);
            if (Q.policy_a) aa = act; else ab = act;
        }
        swar::Out o;
        uint32_t sa = 0u, sb = 0u, cls4 = 0u;
        swar::Rand4 rnd;
        bool listed = false;                                             // SLIPM == 3: the group goes to the exact walk of the per-lane kernel
        if (SLIPM == 3) {
            // The caller's uniforms against the NOMINAL thresholds of the slip list (slip_decide4_f64, soccer_slip.hpp); a group
            // with a lane within 2^-40 of one (or beyond the last threshold) is left to the per-lane kernel's exact walk: listed,
            // nothing stored here.
            const SlipF64& F = *Q.f64;
            const double us[4] = {us0, us1, us2, us3};
            uint32_t c4 = 0u, k4 = 0u; bool near = false;
            SOCCER_SLIP_DECIDE4_F64(F, us, c4, k4, near)
            if (near) {
                const uint32_t slot = atomicAdd(Q.work_count, 1u);
                Q.worklist[slot] = (uint32_t)g;
                listed = true;                                            // nothing of this group is stored or counted here
            }
            swar::slip_moves4(c4, swar::canon4(aa), swar::canon4(ab), sa, sb, cls4);
            rnd = swar::Rand4{k4 << 6, Q.u_reset ? (xr >> Q.C.isd_shift) : (swar::pack_byte0(blk.w[0], blk.w[1], blk.w[2], blk.w[3]) >> Q.C.isd_shift)};
        } else if (SLIP) {
            uint32_t k4 = 0u;
            if (SLIPM == 2) {
                const uint32_t p4 = swar::slip_count4_lut<kSlipStepBucketBits, kSlipStepCompares>(slip_lut, slip_thr, blk.w[0], blk.w[1], blk.w[2], blk.w[3]);
                // the counts need the random words and the table only: the empty statement ties the loaded actions to them, so that
                // the wait for the state loads comes after the table reads and not before
                asm volatile("" : "+v"(aa), "+v"(ab) : "v"(p4));
                swar::slip_from_count4(p4, Q.L.c_off, swar::canon4(aa), swar::canon4(ab), sa, sb, k4, cls4);
            }
            else swar::slip_select4(Q.L, Q.sub, swar::canon4(aa), swar::canon4(ab), blk.w[0], blk.w[1], blk.w[2], blk.w[3], sa, sb, k4, cls4);
            rnd = swar::Rand4{k4 << 6, swar::pack_byte0(blk.w[0], blk.w[1], blk.w[2], blk.w[3]) >> Q.C.isd_shift};
        } else {
            rnd = swar::rand_nibble(Q.C.isd_shift, (uint32_t)tick & 7u, blk.w[0], blk.w[1], blk.w[2], blk.w[3]);
            if (EXPL) {                                              // Rand4: the quarter in bits 7, 6 of each byte; the reset draw, shifted
                if (Q.u_step) rnd.kq = xq << 6;
                if (Q.u_reset) rnd.rs = xr >> Q.C.isd_shift;
            }
        }
        // What the step needs of the actions and the draws alone goes ahead of the state: the actions are the wave's oldest loads,
        // so this runs while the state is still in flight.  (The empty statement ties the state words to it: the scheduler works a
        // block at a time and would otherwise be free to put the wait for the state first.)
        const swar::Moves4 M = swar::step4_moves<SLIP>(Q.C, aa, ab, sa, sb, rnd);
        asm("" : "+v"(S.ra), "+v"(S.ca), "+v"(S.tt) : "v"(M.dra), "v"(M.dca), "v"(M.drb), "v"(M.dcb), "v"(M.ira), "v"(M.irb), "v"(M.ip), "v"(M.bad_action));
        if (LAYOUT == kStatePacked && !POLICY) swar::unpack3(S.ra, S.ca, S.tt, S);
        if (!listed) {
        // Frozen lanes and goal tuples exist only without auto-reset or after a state injection; a thread none of whose lanes is
        // in either condition (nearly every thread of an auto-resetting handle) takes the step without the code for them —
        // 31 vector instructions fewer, 12 for the test: in this kernel every instruction shows (5.6 ns).
        const uint32_t edge = swar::is_zero(S.ca) | swar::is_zero(S.cb) | swar::is_zero(S.ca ^ Q.C.Wm1x4) | swar::is_zero(S.cb ^ Q.C.Wm1x4);
        const bool special = Q.C.autoreset == 0u || (((S.ps << 6) | edge) & swar::K80) != 0u;
        if (special) swar::step4_state<true, FULL, SLIP, GEO>(Q.C, S, M, cls4, rnd, o);
        else swar::step4_state<false, FULL, SLIP, GEO>(Q.C, S, M, cls4, rnd, o);
        uint8_t* sw = const_cast<uint8_t*>(sp);
        // the stores' offset is opaque to the optimiser: it would otherwise hoist the 64-bit addresses of the loads above the
        // branch and reuse them (instruction selection works a block at a time and then no longer sees base + offset)
        uint32_t j0 = i0; asm volatile("" : "+v"(j0));
        const uint32_t j0x2 = j0 << 1, j0x4 = j0 << 2;
#define ATW(base, off) (reinterpret_cast<uint8_t*>(base) + (off))
        if (LAYOUT == kStatePacked) {
            uint32_t pa, pb, pt;
            swar::pack3(S, pa, pb, pt);
            __builtin_nontemporal_store(pa, reinterpret_cast<uint32_t*>(ATW(sw, j0)));
            __builtin_nontemporal_store(pb, reinterpret_cast<uint32_t*>(ATW(sw + state_stride, j0)));
            __builtin_nontemporal_store(pt, reinterpret_cast<uint32_t*>(ATW(sw + 2 * state_stride, j0)));
        } else {
            __builtin_nontemporal_store(S.ra, reinterpret_cast<uint32_t*>(ATW(sw, j0)));
            __builtin_nontemporal_store(S.ca, reinterpret_cast<uint32_t*>(ATW(sw + state_stride, j0)));
            __builtin_nontemporal_store(S.rb, reinterpret_cast<uint32_t*>(ATW(sw + 2 * state_stride, j0)));
            __builtin_nontemporal_store(S.cb, reinterpret_cast<uint32_t*>(ATW(sw + 3 * state_stride, j0)));
            __builtin_nontemporal_store(S.ps, reinterpret_cast<uint32_t*>(ATW(sw + 4 * state_stride, j0)));
            __builtin_nontemporal_store(S.tt, reinterpret_cast<uint32_t*>(ATW(sw + 5 * state_stride, j0)));
        }
        if (o_obs) __builtin_nontemporal_store((unsigned long long)o.obs_lo | ((unsigned long long)o.obs_hi << 32),
                                               reinterpret_cast<unsigned long long*>(ATW(o_obs, j0x2)));
        if (o_reward) __builtin_nontemporal_store(o.rew, reinterpret_cast<uint32_t*>(ATW(o_reward, j0)));
        if (o_term) __builtin_nontemporal_store(o.term, reinterpret_cast<uint32_t*>(ATW(o_term, j0)));
        if (o_trunc) __builtin_nontemporal_store(o.trunc, reinterpret_cast<uint32_t*>(ATW(o_trunc, j0)));
        if (OUT >= 1) {
            if (o_raf || o_rbf) {                                   // the rewards as the floats a gym caller reads (:400-402)
                const int32_t r = (int32_t)o.rew;
                const float f0 = (float)((r << 24) >> 24), f1 = (float)((r << 16) >> 24), f2 = (float)((r << 8) >> 24), f3 = (float)(r >> 24);
                typedef float f4 __attribute__((ext_vector_type(4)));
                if (o_raf) { const f4 va = {f0, f1, f2, f3}; __builtin_nontemporal_store(va, reinterpret_cast<f4*>(ATW(o_raf, j0x4))); }
                if (o_rbf) { const f4 vb = {0.0f - f0, 0.0f - f1, 0.0f - f2, 0.0f - f3};
                             __builtin_nontemporal_store(vb, reinterpret_cast<f4*>(ATW(o_rbf, j0x4))); }
            }
            if (o_fin) __builtin_nontemporal_store(o.term | o.trunc, reinterpret_cast<uint32_t*>(ATW(o_fin, j0)));
            // A's return of the episode that just ended = the reward of its last step (only that step can carry one);
            // lanes whose episode goes on keep what the stream holds.  Rare: one read-modify-write of the thread's own dword.
            if (o_last && (o.finished & swar::K80)) {
                uint32_t* lr = reinterpret_cast<uint32_t*>(ATW(o_last, j0));
                *lr = swar::bfi(swar::mask_of(o.finished), o.rew, *lr);
            }
        }
        if (FULL) {
            if (o_code) __builtin_nontemporal_store(o.code, reinterpret_cast<uint32_t*>(ATW(o_code, j0)));
            if (o_fobs) __builtin_nontemporal_store((unsigned long long)o.fin_lo | ((unsigned long long)o.fin_hi << 32),
                                                         reinterpret_cast<unsigned long long*>(ATW(o_fobs, j0x2)));
            // finished episodes by return: a reward byte is 0x01 / 0xff only on the step that ends the episode
            if (stats) hist.add_totals((uint32_t)__builtin_popcount(o.finished & swar::K80),
                                       (int32_t)__builtin_popcount(o.rew & swar::K01) - 2 * (int32_t)__builtin_popcount(o.rew & swar::K80),
                                       (uint32_t)__builtin_popcount(o.rew & swar::K01));
        }
        if (o.frozen) misuse[0] = 1u;
        if (o.bad_action) misuse[1] = 1u;
        }
        // (published last: a store in flight ahead of the loads' waits would turn them into waits for everything — loads and
        // stores share the wave's counter and complete out of order with respect to each other)
        if (tick_out && blockIdx.x == 0 && threadIdx.x == 0) *tick_out = tick + 1ull;
#undef AT
#undef ATW
    }
    if (stats) hist.flush_at(hist_at, hist_mask);
}

}  // namespace soccer
