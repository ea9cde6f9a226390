// soccer_kernels.hpp — what the gfx950 (CDNA4 / MI355X) kernels share: the argument blocks, Philox, the rule functions of
// one lane (lane_step), the packed lane vectors and the episode histogram.  The kernels themselves are in one header per
// family, each included by exactly one translation unit (the library is built without relocatable device code, so a
// kernel must be emitted once): soccer_step_kernels.hpp, soccer_rollout_kernels.hpp, soccer_env_kernels.hpp (reset, the
// one-environment call, trajectory returns), soccer_planner_kernels.hpp (transition table, planners, minimax),
// soccer_pair_kernels.hpp (the pair evaluators: cross-play, match outcomes, occupancy, policy gradients) and
// soccer_metagame_kernels.hpp (the n_a x n_b matrix games of soccer_solve_meta_games).
//
// What is evaluated per lane, and where the reference states it
// (gym_soccer/envs/soccer_simultaneous_env.py):
//   cell move via the move/bounds table ................ _next_cell          :364-373
//   ordered 5-way collision resolution ................. _get_next_state     :296-362
//   nine slip combinations, float64 weights, zero-skip . :202-227, :241
//   done / reward ...................................... :235-240
//   outcome selection .................................. categorical_sample  :395 (gym 0.26.2)
//   bookkeeping (timestep, truncation, needs_reset) .... :396-406
//   reset from the initial state distribution .......... :410-424
//
// Execution shape: wave64; each thread owns 4 (rollout: E = 1/4/8) consecutive lanes (environments) so
// that every SoA byte stream is read and written with one dword (dwordx2) per thread — 256/512 B per
// wave instruction.  One Philox4x32-10 block serves four consecutive global lanes.
//   step_kernel_hot / step_kernel : one step per launch; rolled lane loop (small code: a launch starts
//                                   with a cold instruction cache); rule tables read through L1/L2
//   rollout_kernel                : T steps per launch with the state in registers; lane loop unrolled;
//                                   rule tables staged in LDS once per workgroup
//   reset_kernel, enumerate_kernel: reset from the ISD; the reference's transition table
// No MFMA: there is no contraction on this path.  By bytes the kernels are HBM-bound (19 B per
// env-step); measured, a single-step launch at 2^20 lanes is bound by launch latency plus ~130 vector
// instructions per lane that do not overlap its load and store phases.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "soccer_games.hpp"
#include "soccer_slip.hpp"
#include "soccer_swar.hpp"

namespace soccer {

constexpr int kBlock = 256;
constexpr int kHistSlots = 16384;        // minimum: >= waves of the largest CAPPED grid (8 blocks x 4 waves x 512 CUs); a handle
                                         // whose byte-parallel step launches more waves than this (n_lanes > 2^22) gets more slots
constexpr int kHistStride = 4;           // u64 per slot: return -1, 0, +1, pad
constexpr int kIsdWords = 16;            // LDS: 4 ISD entries x (A, B, poss|obs<<16, pad)

// How a handle keeps its resident state (soccer_state_streams): six byte streams, or the three of swar::pack3 (handles
// whose pitch packs and that are not host-mapped).  Every kernel that touches the state speaks both.
enum StateLayout : uint32_t { kStateWide = 0u, kStatePacked = 1u };

struct KernelParams {
    // resident state: byte streams back to back, `state_stride` bytes apart.  kStateWide: six, in the order
    // row_a, col_a, row_b, col_b, poss (bit0 possession, bit1 needs_reset), t; kStatePacked: three,
    // poss << 7 | row_a << 4 | col_a, needs_reset << 7 | row_b << 4 | col_b, t
    uint8_t* state;
    unsigned long long state_stride;
    uint32_t state_layout;                // StateLayout
    // rule tables in global memory (staged to LDS)
    const uint16_t* lut;                  // [lut_len] observation index per state tuple
    const uint32_t* next_cell;            // [2][H*W][5]: (has_ball, cell, move) -> (row<<8|col)<<16 | (row*W+col) reached
    const uint32_t* isd;                  // [kIsdWords]
    // single-agent mode: the fixed side's action per observation index (int8[nS]), or nullptr
    const int8_t* policy_a; const int8_t* policy_b;
    // randomness
    const unsigned long long* tick_in;    // device tick slot read by this launch
    unsigned long long* tick_out;         // slot written (tick_in + ticks consumed)
    uint32_t key0, key1;
    unsigned long long lane_offset;
    // statistics
    unsigned long long* hist;             // [hist_mask + 1][4]: one private slot per wave of the grid, bins 0..2
    uint32_t hist_mask;                   // slots - 1 (a power of two >= the waves of the largest grid that counts)
    unsigned int* misuse;                 // sticky flag
    // geometry / constants
    unsigned long long first;             // first lane (within the handle) this launch covers
    unsigned long long n;                 // number of lanes this launch covers
    int32_t W, HW, HW5, nc_len, lut_len;   // HW5 = 5*H*W
    int32_t max_steps;
    uint32_t autoreset;
    uint32_t step_stats;                  // batched_step feeds the episode histogram (SOCCER_F_STEP_STATS)
    uint32_t isd_shift;                   // 2 - log2(n_isd): index = two random bits >> isd_shift
    double w[4];                          // slip-combination weights c0..c3 (:211-222)
    // slip fast path: cumulative weight after each ACTIVE (non-zero) combination in reference order
    // (+inf beyond), their count, and their combination ids packed 4 bits each
    double B[9]; uint32_t nb; unsigned long long act_pack;
    // integer form of the same decision for draws that come from a Philox word (u = (m + 1/2) * 2^-30, m < 2^30):
    // running sum t <= u  <=>  m >= ceil(t * 2^30 - 1/2).  Used only when the host has checked, by walking every list
    // shape, that this integer is the same for every shape at every entry position (soccer_slip.hpp): then it is the
    // reference's decision for every draw and the float64 walk is never needed (slip_int = 1).
    uint32_t CB[9]; uint32_t slip_int;    // 0 float64 only, 1 integer only
    const uint4* sub;                     // [9] per active combination: { t1 (2 outcomes), t1, t2, t3 (4 outcomes) }, as integers
};

struct StepIO {
    const int8_t* act_a; const int8_t* act_b;
    const double* u_step; const double* u_reset;
    uint16_t* obs; int8_t* reward; uint8_t* terminated; uint8_t* truncated;
    uint8_t* prob_code; uint16_t* final_obs; int8_t* last_return;
    float* reward_a_f32; float* reward_b_f32; uint8_t* finished;      // the gym surface's float rewards / terminated | truncated
    // the 4-lane groups step_kernel_swar<.., SLIPM = 3, ..> left to the exact float64 walk (a caller's uniform within 2^-40 of a
    // nominal threshold): the per-lane kernel then steps exactly these groups, zeroes the count and adds to the two uint64
    // statistics 8 bytes behind it (work_count is 8-byte aligned); nullptr: every group
    const uint32_t* worklist; uint32_t* work_count;
};

struct ResetIO {
    const uint8_t* mask; const double* u_reset; uint16_t* obs;
};

struct RolloutIO {
    int32_t n_steps; int32_t sample_actions;
    const uint16_t* mix_a; const uint16_t* mix_b;   // [nS][4] cumulative thresholds (0..32768) of a mixed policy, or nullptr
    const int8_t* act_a; const int8_t* act_b; long long act_stride;
    uint16_t* obs; int8_t* reward; uint8_t* terminated; uint8_t* truncated; long long out_stride;
    int32_t* return_sum; int32_t* episode_count;
    uint16_t* final_obs; uint8_t* prob_code;      // batched_rollout_ex: per-step [T][n] trajectories (row stride out_stride) or nullptr
};

// ---- Philox4x32-10 (Salmon et al. 2011; Random123 constants) ---------------------------------
struct Philox4 { uint32_t w[4]; };

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                 uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        // hi ^ counter ^ key as ONE v_bitop3_b32 (truth table 0x96: three-way xor); the compiler emits two v_xor_b32 for the
        // expression.  -20 of the ~60 vector instructions of a block: +4 % on the fused rollout, +7 % on the self-play rollout
        const uint32_t n0 = __builtin_amdgcn_bitop3_b32((uint32_t)(p1 >> 32), c1, k0, 0x96);
        const uint32_t n2 = __builtin_amdgcn_bitop3_b32((uint32_t)(p0 >> 32), c3, k1, 0x96);
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// the block shared by global lanes 4q .. 4q+3 at `tick`; purpose 0 = step/reset, 1 = sampled actions.
// Callers pass `tick >> 3` for the step/reset block of a slip_prob == 0 handle (one block serves eight ticks).
__device__ __forceinline__ Philox4 lane_block(const KernelParams& P, unsigned long long q,
                                              unsigned long long tick, uint32_t purpose) {
    return philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)tick,
                         (uint32_t)(tick >> 32) | (purpose << 31), P.key0, P.key1);
}

// One lane's randomness for a step: the uniform as float64 (slip lists), floor(4u) (lists whose
// probabilities are dyadic: slip_prob == 0) and two independent bits for the ISD draw.
struct Draw { double u; uint32_t top2; uint32_t reset2; uint32_t m; };   // m = w >> 2 for word draws

// The RNG convention of include/soccer_hip.h, per lane:
//   SLIP (slip_prob > 0): lane word w of the tick's own block: u = ((w >> 2) + 1/2) * 2^-30, reset bits = w & 3
//   otherwise: the lane's word of the block of tick >> 3; this tick's nibble is number (tick & 7) ^ 1 from the least
//   significant end: its two high bits are floor(4u) (u = (that + 1/2) / 4), its two low bits the reset draw
template <bool SLIP>
__device__ __forceinline__ Draw draw_from_word(uint32_t w, unsigned long long tick) {
    if (SLIP) return Draw{((double)(w >> 2) + 0.5) * 0x1.0p-30, w >> 30, w & 3u, w >> 2};
    const uint32_t nib = (w >> (4u * (((uint32_t)tick & 7u) ^ 1u))) & 15u;
    return Draw{((double)(nib >> 2) + 0.5) * 0.25, nib >> 2, nib & 3u, 0u};
}
// the tick a step/reset block is keyed by
template <bool SLIP>
__device__ __forceinline__ unsigned long long block_tick(unsigned long long tick) { return SLIP ? tick : tick >> 3; }
// A caller-supplied uniform.  Values outside [0,1) (and NaN) make every running sum compare
// "not greater", which categorical_sample resolves to index 0 — same as u = 0.
__device__ __forceinline__ double sane_uniform(double u) { return ((u >= 0.0) && (u < 1.0)) ? u : 0.0; }
// The same for the float64 walk over a slip list (slip_prob > 0), whose total may round to 1 + 2^-52: there the reference's
// argmax(cumsum(p) > u) picks the LAST entry for u == 1.0 (np_random.random() never returns it, but a caller's array may hold
// it), so the upper side is left to the walk — which answers index 0 when no running sum exceeds u — and only negative values
// and NaN are folded onto 0 (every first entry is positive: index 0 either way).
__device__ __forceinline__ double sane_uniform_walk(double u) { return (u >= 0.0) ? u : 0.0; }

// ---- LDS-resident rule tables ------------------------------------------------------------------
struct Tables {
    const uint16_t* lut;    // observation index per tuple
    const uint32_t* nc;     // move/bounds table (LDS in the rollout/reset kernels, global in the step kernel)
    const uint32_t* isd;    // initial-state entries
};

// LDS layout (dwords): [0, kIsdWords) ISD, [kIsdWords, kIsdWords + nc_len) move/bounds table, then
// (LUT_LDS) the observation table
template <bool LUT_LDS>
__device__ __forceinline__ Tables stage_tables(const KernelParams& P, uint32_t* smem) {
    if (threadIdx.x < kIsdWords) smem[threadIdx.x] = P.isd[threadIdx.x];
    uint32_t* nc = smem + kIsdWords;
    for (int i = threadIdx.x; i < P.nc_len; i += kBlock) nc[i] = P.next_cell[i];
    Tables T;
    T.isd = smem; T.nc = nc;
    if (LUT_LDS) {
        uint32_t* lut = nc + P.nc_len;
        const int lut_dw = P.lut_len >> 1;                // lut_len is even
        const uint32_t* src = reinterpret_cast<const uint32_t*>(P.lut);
        for (int i = threadIdx.x; i < lut_dw; i += kBlock) lut[i] = src[i];
        T.lut = reinterpret_cast<const uint16_t*>(lut);
    } else {
        T.lut = P.lut;                                    // global (L1/L2)
    }
    __syncthreads();
    return T;
}

// ---- one lane's state in registers -------------------------------------------------------------
// A player's position is carried as one word: low 16 bits the cell id row*W+col (table / LUT index),
// high 16 bits (row<<8 | col) (what the SoA streams store).  Equality of words == equality of cells.
struct Lane {
    uint32_t A, B;      // positions
    uint32_t p;         // possession 0/1
    uint32_t need;      // needs_reset 0/1
    uint32_t t;
};

struct StepResult {
    uint32_t obs, final_obs;
    int32_t reward;
    uint32_t term, trunc, code;
    uint32_t finished;      // episode ended at this step (before any auto-reset)
};

// a*b + c for operands below 2^24: one full-rate v_mad_u32_u24 (a 32-bit a*b+c is a quarter-rate op)
__device__ __forceinline__ uint32_t mad24(uint32_t a, uint32_t b, uint32_t c) { return __umul24(a, b) + c; }

__device__ __forceinline__ uint32_t make_pos(uint32_t row, uint32_t col, int W) {
    return mad24(row, (uint32_t)W, col) | (((row << 8) | col) << 16);
}
__device__ __forceinline__ uint32_t cell_of(uint32_t pos) { return pos & 0xffffu; }
__device__ __forceinline__ uint32_t col_of(uint32_t pos) { return (pos >> 16) & 0xffu; }

// Observation index of a tuple: one gather from the per-tuple table (goal tuples hold 0, :493-494).
// A closed form exists — obs = 1 + 2*(iA*(NI-1) + iB - (iB > iA)) + p over interior-cell indices, see
// Rules::build, which checks the table against it — but the kernels are VALU-bound and the gather
// rides the memory pipe: the ~12 extra vector instructions measured 4 % slower per step.
__device__ __forceinline__ uint32_t obs_of(const Tables& T, const KernelParams& P, uint32_t A, uint32_t B, uint32_t p) {
    return T.lut[(mad24(cell_of(A), (uint32_t)P.HW, cell_of(B)) << 1) | p];
}

// slipped move of an action: variant 0 intended, 1/2 the two orthogonals (:205-206)
//   NOOP->NOOP,NOOP  NORTH->EAST,WEST  SOUTH->WEST,EAST  EAST->SOUTH,NORTH  WEST->NORTH,SOUTH
__device__ __forceinline__ uint32_t slip_move(uint32_t a, int variant) {
    if (variant == 0) return a;
    const uint32_t tab = variant == 1 ? 0x12430u : 0x21340u;
    return (tab >> (4u * a)) & 7u;
}

enum : uint32_t { K_MOVE = 0, K_FLIP = 1, K_COIN = 2, K_FOUR = 3 };

struct Resolved { uint32_t kind, nA, nB; };

// the cell a player reaches with one move (_next_cell :364-373, via the move/bounds table)
__device__ __forceinline__ uint32_t moved(const Tables& T, const KernelParams& P, uint32_t pos, uint32_t has_ball, uint32_t mv) {
    return T.nc[mad24(has_ball, (uint32_t)P.HW5, mad24(cell_of(pos), 5u, mv))];
}

// _get_next_state (:296-362) for a live tuple, given the cells nA / nB the two (possibly slipped) moves
// reach.  aa/ab are the ORIGINAL actions: the reference's NOOP tests use those, not the moves.
__host__ __device__ __forceinline__ Resolved classify(uint32_t A, uint32_t B, uint32_t nA, uint32_t nB, uint32_t aa, uint32_t ab) {
    const bool e1 = nA == B, e2 = nB == A, sA = nA == A, sB = nB == B;
    const bool swap = e1 & e2;                                                         // :315-322
    const bool stander = (e1 & (ab == 0u)) | (e2 & (aa == 0u));                      // :330-331
    const bool bounce = (sA & (aa != 0u) & e2) | (sB & (ab != 0u) & e1);              // :338-339
    const bool same = nA == nB;                                                        // :347
    const uint32_t kind = (swap | (bounce & !stander)) ? (uint32_t)K_COIN
                        : stander ? (uint32_t)K_FLIP : same ? (uint32_t)K_FOUR : (uint32_t)K_MOVE;
    return Resolved{kind, nA, nB};
}

struct Outcome { uint32_t A, B, p, kcode; };

// outcome k of a resolved collision, in the reference's list order
// (:326-327, :335, :343-344, :352-356, :360); branch-free selects on values
__device__ __forceinline__ Outcome pick(uint32_t A, uint32_t B, uint32_t p, const Resolved& R, uint32_t k) {
    const bool mv = R.kind == K_MOVE, fl = R.kind == K_FLIP, four = R.kind == K_FOUR;
    const bool a_moves = mv | (four & (k >= 2u));
    const bool b_moves = mv | (four & (k < 2u));
    Outcome o;
    o.A = a_moves ? R.nA : A;
    o.B = b_moves ? R.nB : B;
    o.p = mv ? p : (fl ? (p ^ 1u) : (k & 1u));
    o.kcode = (mv | fl) ? 0u : (four ? 2u : 1u);
    return o;
}

// Returns true when the lane was stepped while it needed a reset (left untouched; :376).
// WORD: the draw is known to come from a Philox word (d.m valid), which allows the integer slip decision.
// INT_ONLY: the caller has checked P.slip_int on the host; the float64 decision is compiled out.
template <bool SLIP, bool WORD = false, bool INT_ONLY = false>
__device__ __forceinline__ bool lane_step(const Tables& T, const KernelParams& P, Lane& Lref,
                                          uint32_t aa, uint32_t ab, const Draw& d, StepResult& out) {
    const uint32_t A = Lref.A, B = Lref.B, p = Lref.p, t = Lref.t;
    const uint32_t Wm1 = (uint32_t)(P.W - 1);
    const uint32_t carrier_col = col_of(p ? B : A);
    const bool in_goal = (carrier_col == 0u) | (carrier_col == Wm1);   // goal tuple: absorbing (:300-301)
    Outcome sel;
    uint32_t cls = 0;
    if (!SLIP) {
        // single surviving combination, weight 1.0 (:226-227): list probabilities are 1, .5/.5 or .25x4,
        // so the sampled index is floor(2u) / floor(4u)
        const Resolved R = classify(A, B, moved(T, P, A, p ^ 1u, aa), moved(T, P, B, p, ab), aa, ab);
        const uint32_t k = R.kind == K_COIN ? (d.top2 >> 1) : d.top2;
        sel = pick(A, B, p, R, k);
    } else {
        // VA / VB / CLS of the nine combinations (:209-223), 2 bits each: A's move variant, B's move variant and the
        // weight class (c0..c3).  Bit fields, not arrays: a loop the compiler leaves rolled must not turn them
        // (or the by-value weights P.w) into scratch.
        constexpr uint32_t VA2 = 0u | (0u << 2) | (0u << 4) | (1u << 6) | (2u << 8) | (1u << 10) | (1u << 12) | (2u << 14) | (2u << 16);
        constexpr uint32_t VB2 = 0u | (1u << 2) | (2u << 4) | (0u << 6) | (0u << 8) | (1u << 10) | (2u << 12) | (1u << 14) | (2u << 16);
        constexpr uint32_t CL2 = 0u | (1u << 2) | (1u << 4) | (2u << 6) | (2u << 8) | (3u << 10) | (3u << 12) | (3u << 14) | (3u << 16);
        const double w0 = P.w[0], w1 = P.w[1], w2 = P.w[2], w3 = P.w[3];
#define SOCCER_WEIGHT_OF(cl) (((cl) & 2u) ? (((cl) & 1u) ? w3 : w2) : (((cl) & 1u) ? w1 : w0))
        const bool use_int = INT_ONLY || (WORD && P.slip_int != 0u);     // wave-uniform
        if (use_int) {
            // Integer decision (see KernelParams::CB): combination = number of scaled cumulative weights <= m,
            // outcome within it = number of its scaled thresholds <= m.  No float64, no fallback — and the
            // combination is known before the move table is read, so two reads suffice.
            uint32_t idx = 0u;
#pragma unroll
            for (int i = 0; i < 9; ++i) idx += d.m >= P.CB[i] ? 1u : 0u;
            const uint32_t c_i = (uint32_t)((P.act_pack >> (4u * idx)) & 0xfull);
            const uint32_t va = (VA2 >> (2u * c_i)) & 3u, vb = (VB2 >> (2u * c_i)) & 3u;
            cls = (CL2 >> (2u * c_i)) & 3u;
            const uint32_t as = va == 0u ? aa : (((va == 1u ? 0x12430u : 0x21340u) >> (4u * aa)) & 7u);   // slip_move
            const uint32_t bs = vb == 0u ? ab : (((vb == 1u ? 0x12430u : 0x21340u) >> (4u * ab)) & 7u);
            const uint32_t cA = moved(T, P, A, p ^ 1u, as), cB = moved(T, P, B, p, bs);
            Resolved R = classify(A, B, cA, cB, aa, ab);
            R.kind = in_goal ? (uint32_t)K_MOVE : R.kind;
            const uint4 th = P.sub[idx];
            const bool two = R.kind == K_COIN, four = R.kind == K_FOUR;
            const uint32_t k = (((two & (d.m >= th.x)) | (four & (d.m >= th.y))) ? 1u : 0u) +
                               ((four & (d.m >= th.z)) ? 1u : 0u) + ((four & (d.m >= th.w)) ? 1u : 0u);
            sel = pick(A, B, p, R, k);
        } else if constexpr (!INT_ONLY) {
        // the slipped move of variant v as a run-time value (slip_move with a constant v is the same table)
        auto slip_move_rt = [](uint32_t a, uint32_t v) { return v == 0u ? a : (((v == 1u ? 0x12430u : 0x21340u) >> (4u * a)) & 7u); };
        // (1) Fast decision.  The list's running sums are, up to rounding, the cumulative weights of the
        // active combinations (P.B, summed on the host in the reference's order) plus multiples of the
        // combination's own q; the true float64 sums differ from these nominal values by < 1e-14 (at most
        // 36 additions of terms <= 1).  If u is farther than 2^-40 from every nominal threshold it can be
        // compared against, the entry found from the nominal thresholds IS the entry the sequential sum
        // finds.  Otherwise (u on or next to a threshold, or beyond the last one) the lane takes the exact
        // path (2).
        uint32_t idx = 0u; bool near_thr = false; double S = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const double b = P.B[i];                                    // wave-uniform; +inf past the last active one
            const bool ge = d.u >= b;
            idx += ge ? 1u : 0u;
            S = ge ? b : S;
            near_thr |= fabs(d.u - b) < 0x1.0p-40;
        }
        near_thr |= idx >= P.nb;
        uint32_t sel_c = (uint32_t)((P.act_pack >> (4u * idx)) & 0xfull), sel_k = 0u;
        uint32_t cA_sel, cB_sel;                                        // the cells the SELECTED combination's moves reach
        {
            // the fast decision needs the move table for ONE combination: two reads (round 4; it used to fetch the three distinct
            // moves of both players up front for the walk below, six dependent gathers on every lane: 17.1 us per launch at 2^20 lanes)
            const uint32_t va = (VA2 >> (2u * sel_c)) & 3u, vb = (VB2 >> (2u * sel_c)) & 3u, cl = (CL2 >> (2u * sel_c)) & 3u;
            const uint32_t cA = moved(T, P, A, p ^ 1u, slip_move_rt(aa, va));
            const uint32_t cB = moved(T, P, B, p, slip_move_rt(ab, vb));
            cA_sel = cA; cB_sel = cB;
            const uint32_t kind = in_goal ? (uint32_t)K_MOVE : classify(A, B, cA, cB, aa, ab).kind;
            const uint32_t n = kind == K_COIN ? 2u : (kind == K_FOUR ? 4u : 1u);
            const double wq = SOCCER_WEIGHT_OF(cl);
            const double q = wq * (n == 1u ? 1.0 : (n == 2u ? 0.5 : 0.25));
            const double t1 = S + q, t2 = t1 + q, t3 = t2 + q;
            sel_k = (((n > 1u) & (d.u >= t1)) ? 1u : 0u) + (((n > 2u) & (d.u >= t2)) ? 1u : 0u) +
                    (((n > 2u) & (d.u >= t3)) ? 1u : 0u);
            near_thr |= (n > 1u) & (fabs(d.u - t1) < 0x1.0p-40);
            near_thr |= (n > 2u) & (fabs(d.u - t2) < 0x1.0p-40);
            near_thr |= (n > 2u) & (fabs(d.u - t3) < 0x1.0p-40);
        }
        // (2) Exact decision, exactly as categorical_sample walks the list: sequential float64 running sum
        // over the combinations in reference order, each contributing 1, 2 or 4 equal entries; record
        // WHICH entry (combination c, outcome k) is the first to exceed u.
        if (near_thr) {
            // each player has only three distinct moves (intended + two orthogonals): 6 table reads serve all nine combinations
            uint32_t cellA[3], cellB[3];
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                cellA[v] = moved(T, P, A, p ^ 1u, slip_move(aa, v));
                cellB[v] = moved(T, P, B, p, slip_move(ab, v));
            }
            double acc = 0.0;
            bool found = false;
            int first_c = -1;                                           // wave-uniform (weights are)
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                const uint32_t cl_c = (CL2 >> (2 * c)) & 3u;
                const double wgt = SOCCER_WEIGHT_OF(cl_c);
                if (wgt == 0.0) continue;                               // uniform branch (:226-227)
                if (first_c < 0) first_c = c;
                const uint32_t va_c = (VA2 >> (2 * c)) & 3u, vb_c = (VB2 >> (2 * c)) & 3u;
                const uint32_t cA_c = va_c == 0u ? cellA[0] : (va_c == 1u ? cellA[1] : cellA[2]);
                const uint32_t cB_c = vb_c == 0u ? cellB[0] : (vb_c == 1u ? cellB[1] : cellB[2]);
                const uint32_t kind = in_goal ? (uint32_t)K_MOVE : classify(A, B, cA_c, cB_c, aa, ab).kind;
                const uint32_t n = kind == K_COIN ? 2u : (kind == K_FOUR ? 4u : 1u);
                const double q = wgt * (n == 1u ? 1.0 : (n == 2u ? 0.5 : 0.25));   // :241
                const double a1 = acc + q, a2 = a1 + q, a3 = a2 + q, a4 = a3 + q;   // sequential cumsum
                const double end = n == 1u ? a1 : (n == 2u ? a2 : a4);
                const uint32_t k = (d.u >= a1 ? 1u : 0u) + (((n > 1u) & (d.u >= a2)) ? 1u : 0u) +
                                   (((n > 2u) & (d.u >= a3)) ? 1u : 0u);
                const bool here = !found & (end > d.u);
                sel_c = here ? (uint32_t)c : sel_c; sel_k = here ? k : sel_k;
                found |= here;
                acc = end;
            }
            if (!found) { sel_c = (uint32_t)(first_c < 0 ? 0 : first_c); sel_k = 0u; }   // argmax of all-False is 0
            const uint32_t va = (VA2 >> (2u * sel_c)) & 3u, vb = (VB2 >> (2u * sel_c)) & 3u;
            cA_sel = va == 0u ? cellA[0] : (va == 1u ? cellA[1] : cellA[2]);
            cB_sel = vb == 0u ? cellB[0] : (vb == 1u ? cellB[1] : cellB[2]);
        }
#undef SOCCER_WEIGHT_OF
        // the selected combination
        cls = (CL2 >> (2u * sel_c)) & 3u;
        sel = pick(A, B, p, classify(A, B, cA_sel, cB_sel, aa, ab), sel_k);
        }
    }
    sel.A = in_goal ? A : sel.A; sel.B = in_goal ? B : sel.B; sel.p = in_goal ? p : sel.p;
    sel.kcode = in_goal ? 0u : sel.kcode;
    // done / reward (:235-240)
    const uint32_t ncc = col_of(sel.p ? sel.B : sel.A);
    const bool goal_now = (ncc == 0u) | (ncc == Wm1);
    const int32_t reward = (goal_now & !in_goal) ? (ncc == Wm1 ? 1 : -1) : 0;
    const uint32_t tt = t + 1u;                                         // :399
    const uint32_t trunc = tt >= (uint32_t)P.max_steps ? 1u : 0u;      // :404
    const uint32_t done = goal_now ? 1u : 0u;
    const uint32_t need = done | trunc;                                 // :406
    const uint32_t ob_step = obs_of(T, P, sel.A, sel.B, sel.p);      // :397 (goal tuples map to 0)
    out.obs = ob_step; out.final_obs = ob_step; out.reward = reward; out.term = done; out.trunc = trunc;
    out.code = cls * 3u + sel.kcode; out.finished = need;
    Lane L{sel.A, sel.B, sel.p, need, tt};
    if (need && P.autoreset) {                                          // in-step reset (:414-423)
        const uint4 e = *reinterpret_cast<const uint4*>(T.isd + 4u * (d.reset2 >> P.isd_shift));
        L.A = e.x; L.B = e.y; L.p = e.z & 1u; L.t = 0u; L.need = 0u;
        out.obs = e.z >> 16;
    }
    const bool frozen = Lref.need != 0u;
    if (frozen) {                        // rare: a lane that needs reset is left untouched (:376)
        const uint32_t ob = obs_of(T, P, A, B, p);
        out.obs = ob; out.final_obs = ob; out.reward = 0; out.term = in_goal ? 1u : 0u;
        out.trunc = t >= (uint32_t)P.max_steps ? 1u : 0u; out.code = 0u; out.finished = 0u;
        L = Lref;
    }
    Lref = L;
    return frozen;
}

__device__ __forceinline__ void lane_reset(const Tables& T, const KernelParams& P, Lane& L, uint32_t two_bits, uint32_t& ob) {
    const uint4 e = *reinterpret_cast<const uint4*>(T.isd + 4u * (two_bits >> P.isd_shift));
    L.A = e.x; L.B = e.y; L.p = e.z & 1u; L.t = 0u; L.need = 0u;
    ob = e.z >> 16;
}

// ---- E-wide packed byte / halfword vectors -------------------------------------------------------
// E consecutive bytes of one SoA stream, held as E/4 dwords so that element access is a constant
// bit-field extract (no byte arrays: those end up in scratch).  E = 1 is the scalar fallback.
template <int E> struct PackB {
    static constexpr int NW = E / 4;
    uint32_t w[NW];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = 0u;
    }
    __device__ __forceinline__ uint32_t get(int j) const { return (w[j >> 2] >> (8 * (j & 3))) & 0xffu; }
    // v must already fit 8 bits
    __device__ __forceinline__ void put(int j, uint32_t v) { w[j >> 2] |= v << (8 * (j & 3)); }
    __device__ __forceinline__ void load(const void* base, unsigned long long i) {
        const uint8_t* p = static_cast<const uint8_t*>(base) + i;
        if constexpr (E == 4) { w[0] = *reinterpret_cast<const uint32_t*>(p); }
        else { static_assert(E == 8, "E must be 1, 4 or 8");
               const uint2 v = *reinterpret_cast<const uint2*>(p); w[0] = v.x; w[1] = v.y; }
    }
    __device__ __forceinline__ void store(void* base, unsigned long long i) const {
        uint8_t* p = static_cast<uint8_t*>(base) + i;
        if constexpr (E == 4) { *reinterpret_cast<uint32_t*>(p) = w[0]; }
        else { *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]); }
    }
    // streaming variants (trajectory outputs / action inputs: touched once)
    __device__ __forceinline__ void load_nt(const void* base, unsigned long long i) {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(base) + i);
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = __builtin_nontemporal_load(p + k);
    }
    __device__ __forceinline__ void store_nt(void* base, unsigned long long i) const {
        uint32_t* p = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(base) + i);
#pragma unroll
        for (int k = 0; k < NW; ++k) __builtin_nontemporal_store(w[k], p + k);
    }
};
template <> struct PackB<1> {
    uint32_t b;
    __device__ __forceinline__ void clear() { b = 0u; }
    __device__ __forceinline__ uint32_t get(int) const { return b; }
    __device__ __forceinline__ void put(int, uint32_t v) { b = v; }
    __device__ __forceinline__ void load(const void* base, unsigned long long i) { b = static_cast<const uint8_t*>(base)[i]; }
    __device__ __forceinline__ void store(void* base, unsigned long long i) const { static_cast<uint8_t*>(base)[i] = (uint8_t)b; }
    __device__ __forceinline__ void load_nt(const void* base, unsigned long long i) { load(base, i); }
    __device__ __forceinline__ void store_nt(void* base, unsigned long long i) const { store(base, i); }
};

// action bytes as the kernels execute them (swar::canon4); returns non-zero when a byte was outside 0..4
template <int E> __device__ __forceinline__ uint32_t canon_pack(PackB<E>& a) {
    uint32_t bad = 0u;
    if constexpr (E == 1) { const uint32_t c = swar::canon4(a.b & 0xffu); bad = c ^ (a.b & 0xffu); a.b = c; }
    else {
#pragma unroll
        for (int k = 0; k < PackB<E>::NW; ++k) { const uint32_t c = swar::canon4(a.w[k]); bad |= c ^ a.w[k]; a.w[k] = c; }
    }
    return bad;
}

// E consecutive uint16 of one stream, as E/2 dwords; values must already fit 16 bits
template <int E> struct PackH {
    static constexpr int NW = E / 2;
    uint32_t w[NW];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = 0u;
    }
    __device__ __forceinline__ void put(int j, uint32_t v) { w[j >> 1] |= v << (16 * (j & 1)); }
    __device__ __forceinline__ void store(uint16_t* base, unsigned long long i) const {
        uint16_t* p = base + i;
        if constexpr (E == 4) { *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]); }
        else { *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]); }
    }
    __device__ __forceinline__ void store_nt(uint16_t* base, unsigned long long i) const {
        unsigned long long* p = reinterpret_cast<unsigned long long*>(base + i);
#pragma unroll
        for (int k = 0; k < NW; k += 2) __builtin_nontemporal_store((unsigned long long)w[k] | ((unsigned long long)w[k + 1] << 32), p + (k >> 1));
    }
};
template <> struct PackH<1> {
    uint32_t h;
    __device__ __forceinline__ void clear() { h = 0u; }
    __device__ __forceinline__ void put(int, uint32_t v) { h = v; }
    __device__ __forceinline__ void store(uint16_t* base, unsigned long long i) const { base[i] = (uint16_t)h; }
    __device__ __forceinline__ void store_nt(uint16_t* base, unsigned long long i) const { store(base, i); }
};

// E consecutive int32 accumulators (return_sum / episode_count), read-modify-write
template <int E>
__device__ __forceinline__ void add_words(int32_t* base, unsigned long long i, const int32_t (&d)[E]) {
    if constexpr (E == 1) { base[i] += d[0]; }
    else {
#pragma unroll
        for (int k = 0; k < E; k += 4) {
            int4 v = *reinterpret_cast<const int4*>(base + i + k);
            v.x += d[k]; v.y += d[k + 1]; v.z += d[k + 2]; v.w += d[k + 3];
            *reinterpret_cast<int4*>(base + i + k) = v;
        }
    }
}

// the six state streams of E lanes, still packed as loaded (so the loads can be issued early)
template <int E>
struct RawState {
    PackB<E> ra, ca, rb, cb, ps, tt;
    __device__ __forceinline__ void load(const KernelParams& P, unsigned long long i) {
        const uint8_t* s = P.state;
        if (P.state_layout == kStatePacked) {                       // wave-uniform
            PackB<E> a, b;
            a.load(s, i); b.load(s + P.state_stride, i); tt.load(s + 2 * P.state_stride, i);
            if constexpr (E == 1) { swar::Group G; swar::unpack3(a.b, b.b, tt.b, G); ra.b = G.ra; ca.b = G.ca; rb.b = G.rb; cb.b = G.cb; ps.b = G.ps; }
            else {
#pragma unroll
                for (int k = 0; k < PackB<E>::NW; ++k) {
                    swar::Group G; swar::unpack3(a.w[k], b.w[k], tt.w[k], G);
                    ra.w[k] = G.ra; ca.w[k] = G.ca; rb.w[k] = G.rb; cb.w[k] = G.cb; ps.w[k] = G.ps;
                }
            }
            return;
        }
        ra.load(s, i); ca.load(s + P.state_stride, i); rb.load(s + 2 * P.state_stride, i);
        cb.load(s + 3 * P.state_stride, i); ps.load(s + 4 * P.state_stride, i); tt.load(s + 5 * P.state_stride, i);
    }
};

template <int E>
struct LaneVec {
    Lane L[E];
    __device__ __forceinline__ void unpack(const KernelParams& P, const RawState<E>& r) {
#pragma unroll
        for (int j = 0; j < E; ++j) {
            L[j].A = make_pos(r.ra.get(j), r.ca.get(j), P.W);
            L[j].B = make_pos(r.rb.get(j), r.cb.get(j), P.W);
            const uint32_t f = r.ps.get(j);
            L[j].p = f & 1u; L[j].need = (f >> 1) & 1u; L[j].t = r.tt.get(j);
        }
    }
    __device__ __forceinline__ void load(const KernelParams& P, unsigned long long i) {
        RawState<E> r; r.load(P, i); unpack(P, r);
    }
    __device__ __forceinline__ void store(const KernelParams& P, unsigned long long i) const {
        PackB<E> ra, ca, rb, cb, ps, tt;
        ra.clear(); ca.clear(); rb.clear(); cb.clear(); ps.clear(); tt.clear();
#pragma unroll
        for (int j = 0; j < E; ++j) {
            ra.put(j, L[j].A >> 24); ca.put(j, (L[j].A >> 16) & 0xffu);
            rb.put(j, L[j].B >> 24); cb.put(j, (L[j].B >> 16) & 0xffu);
            ps.put(j, L[j].p | (L[j].need << 1)); tt.put(j, L[j].t);
        }
        uint8_t* s = P.state;
        if (P.state_layout == kStatePacked) {                       // wave-uniform
            PackB<E> a, b;
            if constexpr (E == 1) { uint32_t t_; swar::pack3(swar::Group{ra.b, ca.b, rb.b, cb.b, ps.b, tt.b}, a.b, b.b, t_); }
            else {
#pragma unroll
                for (int k = 0; k < PackB<E>::NW; ++k) { uint32_t t_; swar::pack3(swar::Group{ra.w[k], ca.w[k], rb.w[k], cb.w[k], ps.w[k], tt.w[k]}, a.w[k], b.w[k], t_); }
            }
            a.store(s, i); b.store(s + P.state_stride, i); tt.store(s + 2 * P.state_stride, i);
            return;
        }
        ra.store(s, i); ca.store(s + P.state_stride, i); rb.store(s + 2 * P.state_stride, i);
        cb.store(s + 3 * P.state_stride, i); ps.store(s + 4 * P.state_stride, i); tt.store(s + 5 * P.state_stride, i);
    }
};

// episode histogram: per-thread counts, one DPP wave reduction at exit, one atomic per bin per wave
// on a sharded global array (no LDS, no workgroup barrier)
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true);    // quad_perm [1,0,3,2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true);    // quad_perm [2,3,0,1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, true);   // row_half_mirror
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, true);   // row_mirror
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}

// EARLY: fetch the wave's slot at kernel entry so the load's latency hides under the whole kernel (the
// single-step kernel, where every microsecond of tail counts); otherwise read-modify-write at exit
// (the rollout kernel, which would pay 6 live VGPRs — and an occupancy step — for nothing).
template <bool EARLY>
struct HistAcc {
    uint32_t fin, pos, neg;     // this thread's finished episodes: all / return +1 / return -1
    ulonglong2 old01; unsigned long long old2;   // EARLY only: the wave's slot as of kernel entry (lane 0)
    __device__ __forceinline__ unsigned long long* slot_at(unsigned long long* base, uint32_t mask) const {
        const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        return base + (size_t)(wave & mask) * kHistStride;
    }
    // Every wave of a launch owns one slot — the host sizes the array to the largest grid that counts (soccer_create) —
    // and launches are stream-ordered, so plain loads and stores accumulate without atomics.
    __device__ __forceinline__ void init_at(unsigned long long* base, uint32_t mask) {
        fin = 0u; pos = 0u; neg = 0u;
        if (EARLY) {
            old01 = make_ulonglong2(0ull, 0ull); old2 = 0ull;
            if ((threadIdx.x & 63u) == 0u) {
                const unsigned long long* h = slot_at(base, mask);
                old01 = *reinterpret_cast<const ulonglong2*>(h); old2 = h[2];
            }
        }
    }
    __device__ __forceinline__ void init(const KernelParams& P) { init_at(P.hist, P.hist_mask); }
    __device__ __forceinline__ void add(uint32_t finished, int32_t reward) {
        fin += finished; pos += reward > 0 ? 1u : 0u; neg += reward < 0 ? 1u : 0u;
    }
    // totals of a whole group at once: `finished` episodes, sum of their rewards and of |reward|
    // (rewards are -1/0/+1, and only the step that ends an episode can carry one)
    __device__ __forceinline__ void add_totals(uint32_t finished, int32_t reward_sum, uint32_t nonzero) {
        fin += finished; pos += (nonzero + (uint32_t)reward_sum) >> 1; neg += (nonzero - (uint32_t)reward_sum) >> 1;
    }
    // Call once at kernel exit, where every lane of the wave is active.
    __device__ __forceinline__ void flush(const KernelParams& P) { flush_at(P.hist, P.hist_mask); }
    __device__ __forceinline__ void flush_at(unsigned long long* base, uint32_t mask) {
        const uint32_t tot = wave_sum(fin), p = wave_sum(pos), n = wave_sum(neg);
        if ((threadIdx.x & 63u) == 0u && tot) {
            unsigned long long* h = slot_at(base, mask);
            if (!EARLY) { old01 = *reinterpret_cast<const ulonglong2*>(h); old2 = h[2]; }
            *reinterpret_cast<ulonglong2*>(h) = make_ulonglong2(old01.x + n, old01.y + (tot - p - n));
            h[2] = old2 + p;
        }
    }
};

__device__ __forceinline__ void publish_tick(const KernelParams& P, unsigned long long tick, unsigned long long used) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *P.tick_out = tick + used;
}

// random words of the E lanes starting at global lane g0 (one Philox block per 4 aligned lanes)
template <int E>
__device__ __forceinline__ void lane_words(const KernelParams& P, unsigned long long g0, unsigned long long tick,
                                           uint32_t purpose, uint32_t (&w)[E]) {
    if (E >= 4 && (g0 & 3ull) == 0ull) {                // wave-uniform: lane_offset % 4 == 0
#pragma unroll
        for (int k = 0; k < E; k += 4) {
            const Philox4 b = lane_block(P, (g0 + k) >> 2, tick, purpose);
#pragma unroll
            for (int j = 0; j < 4 && k + j < E; ++j) w[k + j] = b.w[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const unsigned long long g = g0 + j;
            const Philox4 b = lane_block(P, g >> 2, tick, purpose);
            const uint32_t s = (uint32_t)g & 3u;
            w[j] = s & 2u ? (s & 1u ? b.w[3] : b.w[2]) : (s & 1u ? b.w[1] : b.w[0]);
        }
    }
}

// lanes per step_kernel_swar / rollout_swar_kernel launch: their byte offsets are 32-bit
constexpr unsigned long long kSwarLaunchLanes = 1ull << 30;   // 4 bytes per lane (the float rewards) * 2^30 lanes: offsets below 2^32

}  // namespace soccer
