// soccer_env_kernels.hpp — reset_kernel / reset_kernel_swar, scalar_kernel and trajectory_returns_kernel.
// Included by soccer_hip.hip only: every kernel is emitted by exactly one translation unit.
#pragma once
#include "soccer_kernels.hpp"

namespace soccer {

// =================================================================================================
// batched_reset
// =================================================================================================
template <bool LUT_LDS, bool SLIP>
__global__ __launch_bounds__(kBlock) void reset_kernel(const KernelParams P, const ResetIO IO) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const Tables T = stage_tables<LUT_LDS>(P, smem);
    const unsigned long long tick = *P.tick_in;
    if (P.tick_out) publish_tick(P, tick, 1ull);
    for (unsigned long long k = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; k < P.n;
         k += (unsigned long long)gridDim.x * kBlock) {
        const unsigned long long i = P.first + k;                   // the launch covers lanes [first, first + n)
        const bool sel = IO.mask == nullptr || IO.mask[i] != 0;
        uint32_t ob = 0u;
        if (sel) {
            uint32_t bits;
            if (IO.u_reset) bits = (uint32_t)(sane_uniform(IO.u_reset[i]) * 4.0);
            else { uint32_t w[1]; lane_words<1>(P, P.lane_offset + i, block_tick<SLIP>(tick), 0u, w); bits = draw_from_word<SLIP>(w[0], tick).reset2; }
            LaneVec<1> S; lane_reset(T, P, S.L[0], bits, ob);
            S.store(P, i);
        } else if (IO.obs) {
            LaneVec<1> S; S.load(P, i);
            ob = obs_of(T, P, S.L[0].A, S.L[0].B, S.L[0].p);
        }
        if (IO.obs) IO.obs[i] = (uint16_t)ob;
    }
}

// batched_reset, byte-parallel (Philox draws, dword-aligned streams, pitches that fit the byte arithmetic): four lanes per
// thread, the state's dword stores (3 packed, 6 wide) + one 8-byte observation store; MASKED also reads the state dwords and
// the mask dword.
struct ResetSwar {
    swar::Consts C;
    uint8_t* state; unsigned long long state_stride; uint32_t layout;      // StateLayout (wave-uniform branches below)
    unsigned long long n, lane_offset;
    const unsigned long long* tick_in; unsigned long long* tick_out;
    uint32_t key0, key1;
    const uint8_t* mask; uint16_t* obs;
};
template <bool MASKED, bool SLIP>
__global__ __launch_bounds__(kBlock) void reset_kernel_swar(const ResetSwar R) {
    const unsigned long long g = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    const unsigned long long i0 = g << 2;
    if (i0 >= R.n) return;                                          // n is a multiple of 4 here; the first lane is 0
    uint8_t* sp = R.state + i0;
    swar::Group S{0u, 0u, 0u, 0u, 0u, 0u};
    uint32_t mask4 = 0u;
    const bool packed = R.layout == kStatePacked;
    if (MASKED) {
        if (packed) {
            swar::unpack3(*reinterpret_cast<const uint32_t*>(sp), *reinterpret_cast<const uint32_t*>(sp + R.state_stride),
                          *reinterpret_cast<const uint32_t*>(sp + 2 * R.state_stride), S);
        } else {
        S.ra = *reinterpret_cast<const uint32_t*>(sp); S.ca = *reinterpret_cast<const uint32_t*>(sp + R.state_stride);
        S.rb = *reinterpret_cast<const uint32_t*>(sp + 2 * R.state_stride); S.cb = *reinterpret_cast<const uint32_t*>(sp + 3 * R.state_stride);
        S.ps = *reinterpret_cast<const uint32_t*>(sp + 4 * R.state_stride); S.tt = *reinterpret_cast<const uint32_t*>(sp + 5 * R.state_stride);
        }
        mask4 = *reinterpret_cast<const uint32_t*>(R.mask + i0);
    }
    const unsigned long long tick = *R.tick_in;
    if (blockIdx.x == 0 && threadIdx.x == 0) *R.tick_out = tick + 1ull;
    if (!MASKED && packed) *reinterpret_cast<uint32_t*>(sp + 2 * R.state_stride) = 0u;      // the timestep needs no draw
    if (!MASKED && !packed) {      // what a reset of every lane writes without a draw — both columns, the timestep — leaves before the Philox block
        *reinterpret_cast<uint32_t*>(sp + R.state_stride) = R.C.isd_ca4; *reinterpret_cast<uint32_t*>(sp + 3 * R.state_stride) = R.C.isd_cb4;
        *reinterpret_cast<uint32_t*>(sp + 5 * R.state_stride) = 0u;
    }
    const unsigned long long q = (R.lane_offset + i0) >> 2;
    const unsigned long long bt = block_tick<SLIP>(tick);
    const Philox4 blk = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)bt, (uint32_t)(bt >> 32), R.key0, R.key1);
    uint32_t o_lo, o_hi;
    const swar::Rand4 rnd = SLIP ? swar::rand_words(R.C.isd_shift, blk.w[0], blk.w[1], blk.w[2], blk.w[3])
                                 : swar::rand_nibble(R.C.isd_shift, (uint32_t)tick & 7u, blk.w[0], blk.w[1], blk.w[2], blk.w[3]);
    swar::reset4<MASKED>(R.C, S, mask4, rnd, o_lo, o_hi);
    if (packed) {
        uint32_t pa, pb, pt;
        swar::pack3(S, pa, pb, pt);
        *reinterpret_cast<uint32_t*>(sp) = pa; *reinterpret_cast<uint32_t*>(sp + R.state_stride) = pb;
        if (MASKED) *reinterpret_cast<uint32_t*>(sp + 2 * R.state_stride) = pt;
    } else {
    *reinterpret_cast<uint32_t*>(sp) = S.ra; *reinterpret_cast<uint32_t*>(sp + 2 * R.state_stride) = S.rb;
    *reinterpret_cast<uint32_t*>(sp + 4 * R.state_stride) = S.ps;
    if (MASKED) {
        *reinterpret_cast<uint32_t*>(sp + R.state_stride) = S.ca; *reinterpret_cast<uint32_t*>(sp + 3 * R.state_stride) = S.cb;
        *reinterpret_cast<uint32_t*>(sp + 5 * R.state_stride) = S.tt;
    }
    }
    if (R.obs) *reinterpret_cast<uint2*>(R.obs + i0) = make_uint2(o_lo, o_hi);
}

// =================================================================================================
// one environment, one step or reset, lowest latency (the single-env facade's path; reference :375-424)
// =================================================================================================
// Inputs arrive BY VALUE as kernel arguments and the results leave as ONE 16-byte store to a host-mapped
// record the host polls: the GPU reads no host memory and the host never enters a stream synchronisation
// (tools/labs/latency_lab.hip: 7.9 us for launch + kernel-written flag + poll against 12.6 us for launch +
// hipStreamSynchronize).  The lane's resident state streams are updated too.
struct ScalarIO {
    uint32_t pos;       // row_a | col_a << 8 | row_b << 16 | col_b << 24
    uint32_t misc;      // poss | t << 8 | act_a << 16 | act_b << 24
    uint32_t op;        // 0 step, 1 reset
    uint32_t seq;       // written to record.x last
    double u_step, u_reset;
    uint4* record;      // host-mapped: { seq, obs | (reward & 0xff) << 16 | term << 24 | trunc << 25 | code << 26,
                        //                next pos (as `pos`), poss | needs_reset << 1 | t << 8 | check << 16 | (seq & 0xff) << 24 }
                        //                check = byte-sum of words 1 and 2 (a torn record is never taken for a complete one)
};

template <bool SLIP>
__global__ __launch_bounds__(64) void scalar_kernel(const KernelParams P, const ScalarIO IO) {
    if (threadIdx.x != 0) return;
    Tables T; T.lut = P.lut; T.nc = P.next_cell; T.isd = P.isd;
    Lane L; StepResult R;
    R.obs = 0u; R.final_obs = 0u; R.reward = 0; R.term = 0u; R.trunc = 0u; R.code = 0u; R.finished = 0u;
    if (IO.op == 1u) {
        uint32_t ob = 0u;
        lane_reset(T, P, L, (uint32_t)(sane_uniform(IO.u_reset) * 4.0), ob);
        R.obs = ob;
    } else {
        L.A = make_pos(IO.pos & 0xffu, (IO.pos >> 8) & 0xffu, P.W);
        L.B = make_pos((IO.pos >> 16) & 0xffu, IO.pos >> 24, P.W);
        L.p = IO.misc & 1u; L.need = 0u; L.t = (IO.misc >> 8) & 0xffu;
        uint32_t a_now = (IO.misc >> 16) & 0xffu, b_now = IO.misc >> 24;
        if (P.policy_a || P.policy_b) {                             // the fixed side acts on the current observation
            const uint32_t s_now = obs_of(T, P, L.A, L.B, L.p);
            if (P.policy_a) a_now = (uint32_t)(uint8_t)P.policy_a[s_now];
            if (P.policy_b) b_now = (uint32_t)(uint8_t)P.policy_b[s_now];
        }
        const double u = sane_uniform(IO.u_step);
        const Draw d{SLIP ? sane_uniform_walk(IO.u_step) : u, (uint32_t)(u * 4.0), (uint32_t)(sane_uniform(IO.u_reset) * 4.0), 0u};
        (void)lane_step<SLIP>(T, P, L, a_now, b_now, d, R);
    }
    { LaneVec<1> S; S.L[0] = L; S.store(P, 0ull); }             // the handle's one lane, in its layout
    const uint32_t res = R.obs | (((uint32_t)R.reward & 0xffu) << 16) | (R.term << 24) | (R.trunc << 25) | (R.code << 26);
    const uint32_t npos = (L.A >> 24) | (((L.A >> 16) & 0xffu) << 8) | ((L.B >> 24) << 16) | (((L.B >> 16) & 0xffu) << 24);
    __threadfence_system();                 // the resident state before the record
    // one 16-byte store = one write transaction; the sequence number opens it, its low byte closes it and word 3 carries a
    // check byte over words 1 and 2, so the host can tell a complete record from a torn one without a second fence (a second fence would put a PCIe
    // round trip on the critical path: +1.6 us per step, measured)
    uint32_t check = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) check += ((res >> (8 * q)) & 0xffu) + ((npos >> (8 * q)) & 0xffu);
    *IO.record = make_uint4(IO.seq, res, npos, L.p | (L.need << 1) | (L.t << 8) | ((check & 0xffu) << 16) | (IO.seq << 24));
    // the call consumes one tick like every batched_* call; nothing above needed its value (the uniforms are the
    // caller's), so its cache miss stays off the path to the record
    *P.tick_out = *P.tick_in + 1ull;
}

// =================================================================================================
// episode returns from result trajectories (soccer_trajectory_returns)
// =================================================================================================
// What the caller of T batched_step calls (or of one batched_rollout) holds afterwards is [T][n] reward / terminated / truncated
// streams; what BASELINE config 4 gathers over xGMI is ONE value per lane — player A's return of the lane's most recently
// finished episode (= the reward of the step that ended it: only that step can carry one, :235-240) — plus the 3-bin histogram
// of all finished episodes.  One pass over the three streams, 3 B per env-step read, 1 (+4) B per lane written: HBM-bound.
// VEC: four lanes per thread by dword (streams 4-aligned, stride % 4 == 0); otherwise a lane per thread by byte.
struct TrajIO {
    const int8_t* reward; const uint8_t* terminated; const uint8_t* truncated;
    long long stride; int32_t n_steps; unsigned long long n;
    int8_t* last_return; int32_t* episode_count;       // nullable
    unsigned long long* hist; uint32_t slot0;           // device u64[slots][4]: per-workgroup counts of returns -1, 0, +1, from slot `slot0`
};
template <bool VEC>
__global__ __launch_bounds__(kBlock) void trajectory_returns_kernel(const TrajIO IO) {
    uint32_t fin_t = 0u, nz_t = 0u, neg_t = 0u;
    const unsigned long long units = VEC ? (IO.n >> 2) : IO.n;
    for (unsigned long long g = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; g < units;
         g += (unsigned long long)gridDim.x * kBlock) {
        if (VEC) {
            const unsigned long long i0 = g << 2;
            uint32_t last = 0u, c8 = 0u, cnt[4] = {0u, 0u, 0u, 0u};
            // eight rows in flight per thread (24 independent dword loads, streamed once: non-temporal; the scheduling barrier
            // keeps them ahead of the arithmetic): a load per row and wait ran at 1.2 TB/s (profiles/r04_a: 174 us for T = 64)
            constexpr int U = 8;
            auto row_of = [&](uint32_t r, uint32_t f) {
                const uint32_t nz = ((f | ((f & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u) >> 7;     // 0 / 1 per byte
                const uint32_t m = nz * 255u, rm = r & m;
                last = (last & ~m) | rm;
                c8 += nz;
                fin_t += (uint32_t)__builtin_popcount(nz); nz_t += (uint32_t)__builtin_popcount(rm & 0x01010101u);
                neg_t += (uint32_t)__builtin_popcount(rm & 0x80808080u);
            };
            int s0 = 0;
            for (; s0 + U <= IO.n_steps; s0 += U) {
                uint32_t r[U], ft[U], fr[U];
#pragma unroll
                for (int k = 0; k < U; ++k) {
                    const long long row = (long long)(s0 + k) * IO.stride;
                    r[k] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(IO.reward + row + i0));
                    ft[k] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(IO.terminated + row + i0));
                    fr[k] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(IO.truncated + row + i0));
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < U; ++k) row_of(r[k], ft[k] | fr[k]);
                if ((s0 & 127) == 120) { for (int j = 0; j < 4; ++j) cnt[j] += (c8 >> (8 * j)) & 0xffu; c8 = 0u; }   // every 128 rows: no byte overflows
            }
            for (; s0 < IO.n_steps; ++s0) {                                              // the last n_steps % 8 rows (c8 gains < 8 here)
                const long long row = (long long)s0 * IO.stride;
                row_of(*reinterpret_cast<const uint32_t*>(IO.reward + row + i0),
                       *reinterpret_cast<const uint32_t*>(IO.terminated + row + i0) | *reinterpret_cast<const uint32_t*>(IO.truncated + row + i0));
            }
            for (int j = 0; j < 4; ++j) cnt[j] += (c8 >> (8 * j)) & 0xffu;
            if (IO.last_return) *reinterpret_cast<uint32_t*>(IO.last_return + i0) = last;
            if (IO.episode_count) *reinterpret_cast<int4*>(IO.episode_count + i0) = make_int4((int)cnt[0], (int)cnt[1], (int)cnt[2], (int)cnt[3]);
        } else {
            int8_t last = 0; uint32_t cnt = 0u;
            for (int s = 0; s < IO.n_steps; ++s) {
                const long long row = (long long)s * IO.stride;
                const int8_t r = IO.reward[row + g];
                if (IO.terminated[row + g] | IO.truncated[row + g]) {
                    last = r; ++cnt; ++fin_t; nz_t += r != 0 ? 1u : 0u; neg_t += r < 0 ? 1u : 0u;
                }
            }
            if (IO.last_return) IO.last_return[g] = last;
            if (IO.episode_count) IO.episode_count[g] = (int32_t)cnt;
        }
    }
    // one private slot per workgroup, summed by the host (atomics of 4 096 waves on three words of one line were 120 of the
    // 170 us this kernel took at T = 64: profiles/r04_a_kernel_stats_other.csv)
    __shared__ uint32_t part[kBlock / 64][3];
    const uint32_t tot = wave_sum(fin_t), nzs = wave_sum(nz_t), neg = wave_sum(neg_t);
    if ((threadIdx.x & 63u) == 0u) { part[threadIdx.x >> 6][0] = neg; part[threadIdx.x >> 6][1] = tot - nzs; part[threadIdx.x >> 6][2] = nzs - neg; }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long v = 0ull;
        for (int wv = 0; wv < kBlock / 64; ++wv) v += part[wv][threadIdx.x];
        IO.hist[(size_t)(IO.slot0 + blockIdx.x) * 4 + threadIdx.x] = v;
    }
}

}  // namespace soccer
