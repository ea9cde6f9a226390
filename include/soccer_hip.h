/*
 * soccer_hip.h — C ABI of libsoccer_hip.so
 *
 * MI355X (gfx950) batched implementation of the step/reset hot path of the
 * Littman-94 grid-soccer Markov game, i.e. of
 *     SoccerSimultaneousEnv.step   (gym_soccer/envs/soccer_simultaneous_env.py:375-408)
 *     SoccerSimultaneousEnv.reset  (gym_soccer/envs/soccer_simultaneous_env.py:410-424)
 * of mimoralea/gym-soccer-littman94, plus the constructor-time rule functions
 * that give those two their meaning (:60-61, :63-109, :146-165, :202-256,
 * :296-362, :364-373).  The reference has no FFI of its own (it is pure
 * Python); these are the entry points a ctypes binding inside that file would
 * call — see INTEGRATION.md for the stub.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; no exception crosses
 *     the ABI.  soccer_last_error(h) gives the message (h may be NULL for
 *     errors raised before a handle exists).
 *   - "lane" = one environment instance.  A handle owns the resident state of
 *     n_lanes lanes on ONE device, a HIP stream and the staged rule tables.
 *   - unless a parameter says "host", array pointers are DEVICE pointers to
 *     caller-owned buffers of n_lanes elements; all work is enqueued on the
 *     handle's stream and is asynchronous (soccer_sync to wait).
 *   - one handle per host thread; calls on one handle are serialised by its
 *     stream.
 *   - state is structure-of-arrays in HBM: row_a,col_a,row_b,col_b int8[n],
 *     poss uint8[n] (bit0: 0 = A has the ball, 1 = B; bit1: lane needs reset),
 *     t uint8[n] (steps taken in the episode, 0..max_steps).
 *
 * Randomness (replaces the reference's per-env np.random.RandomState,
 * :57-58, consumed once per step and once per reset through gym's
 * categorical_sample, :395, :414):
 *   every batched_reset / batched_step call consumes one "tick" k of the handle (a T-step rollout consumes T).
 *   Four consecutive GLOBAL lanes share Philox4x32-10 blocks:
 *       g = lane_offset + i,  q = g >> 2,  key = (seed & 0xffffffff, seed >> 32)
 *       block(c, purpose) = philox4x32_10(counter = (q & 0xffffffff, q >> 32, c & 0xffffffff, (c >> 32) | purpose << 31), key)
 *   (purpose 0: step/reset, 1: in-kernel action sampling; k < 2^63) and lane g owns word w = block[g & 3].
 *   One more block, for the populations with a league opponent alone: block(2^62 + k, 1), the kick-off draw of a league
 *   policy at tick k (same quad, same word rule).  While k < 2^62 it is no block that a step, a reset or an action draw
 *   of any tick takes, so it collides with nothing; soccer_q_population_run refuses a league run that would cross 2^62.
 *   A uniform is always u = (m + 1/2) * 2^-b for a b-bit integer m — never 0, never on a dyadic threshold:
 *     slip_prob > 0   one block per tick, block(k, 0):
 *         step uniform   u = ((w >> 2) + 1/2) * 2^-30      (30 bits)
 *         reset uniform  u = ((w & 3) + 1/2) / 4           (the ISD has 2 or 4 equiprobable entries, :146-165)
 *     slip_prob == 0  every list probability is 1, 1/2 or 1/4 (:326-360), so a step needs floor(4u) and nothing else:
 *       ONE block serves EIGHT ticks, block(k >> 3, 0); tick k takes nibble number (k & 7) ^ 1 of w, counted from the
 *       least significant end:   nib = (w >> (4 * ((k & 7) ^ 1))) & 15
 *         step uniform   u = ((nib >> 2) + 1/2) / 4
 *         reset uniform  u = ((nib & 3) + 1/2) / 4
 *       (ABI 3.  The fused rollout is bound by vector issue, and a Philox block per step was a third of it.)
 *   So results depend on (seed, global lane id, tick) only — never on the
 *   device count or the launch geometry.  Callers that want to feed their own
 *   uniforms (e.g. the single-env facade, which keeps the reference's MT19937
 *   stream on the host) pass u_step / u_reset arrays instead.
 *   Outcome selection is the reference's: first index whose sequential
 *   float64 running sum of list probabilities exceeds u, index 0 if none does.
 */
#ifndef SOCCER_HIP_H
#define SOCCER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SOCCER_ABI_VERSION 3      /* 2: soccer_step_args grew reward_a_f32 / reward_b_f32 / finished
                                     3: the bits -> uniform convention above (half-step offset; eight ticks per block at slip_prob == 0)
                                     (still 3: soccer_trajectory_returns, soccer_comm_*, batched_rollout_ex, soccer_solve_matrix_games,
                                     soccer_minimax_backup, soccer_minimax_value_iteration, soccer_minimax_q_*, soccer_q_learner_*, soccer_wolf_phc_*, soccer_q_population_* (soccer_q_population_create_league and soccer_q_population_league_* among them), soccer_wolf_population_*, soccer_minimax_q_population_*, soccer_best_response, soccer_evaluate_policies, soccer_cross_play, soccer_match_outcomes, soccer_occupancy, soccer_policy_gradient, soccer_gradient_play_*, soccer_solve_meta_games and soccer_rollout_shape were ADDED, captured sequences may hold an odd
                                     number of calls, and a caller's u >= 1 on a slip list follows the reference's comparison — nothing a
                                     round-3 caller relied on changed, and checkpoints record this number for the RNG convention alone) */

/* error codes */
#define SOCCER_OK            0
#define SOCCER_E_INVALID    -1   /* bad argument / config (the reference's AssertionError cases) */
#define SOCCER_E_HIP        -2   /* a HIP runtime call failed */
#define SOCCER_E_NOMEM      -3
#define SOCCER_E_STATE      -4   /* call not valid in the handle's current state (e.g. capture) */

/* cfg.flags */
#define SOCCER_F_AUTORESET   1u  /* lanes that terminate/truncate are reset inside the same step */
#define SOCCER_F_NULL_STREAM 2u  /* enqueue on the device's default (null) stream; cfg.stream ignored */
#define SOCCER_F_STEP_STATS  8u  /* batched_step also feeds the episode histogram (soccer_get_stats); off by
                                    default: it costs ~5 % of a launch.  batched_rollout always counts. */
#define SOCCER_F_HOST_MAPPED 4u  /* small handles (single-env facade): state and staging live in pinned host memory
                                    the GPU reads/writes in place, so the *_host calls and state access copy nothing */
#define SOCCER_F_STREAM_ACTIONS 16u /* batched_step reads its action streams with the non-temporal hint: for callers that
                                    walk through action data larger than the Infinity Cache once (long pre-generated
                                    trajectories).  Unset (default): plain loads, which is faster when the buffers a step
                                    reads were written or read a few steps ago (the loop of an RL agent; a short captured
                                    sequence that is replayed) and slower when they stream in from HBM. */

/* actions (soccer_simultaneous_env.py:8-12); moves are (dcol,drow) (:24-30) */
#define SOCCER_NOOP  0
#define SOCCER_NORTH 1
#define SOCCER_SOUTH 2
#define SOCCER_EAST  3
#define SOCCER_WEST  4

typedef struct soccer_handle soccer_handle;
typedef struct soccer_graph  soccer_graph;

/* Constructor arguments: SoccerSimultaneousEnv.__init__(width, height, slip_prob, ..., seed)
 * (soccer_simultaneous_env.py:35) + the batching parameters the reference does not have. */
typedef struct soccer_config {
    uint64_t n_lanes;       /* environments resident on this handle (>=1) */
    int32_t  width;         /* pitch columns WITHOUT the two goal columns, >=5 (:45) */
    int32_t  height;        /* pitch rows, >=4 (:46) */
    double   slip_prob;     /* [0,1] (:50) */
    int32_t  max_steps;     /* truncation limit; the reference hard-codes 100 (:404). 1..250 */
    int32_t  device;        /* HIP device ordinal */
    uint64_t seed;          /* Philox key */
    uint64_t lane_offset;   /* global id of lane 0 (multi-GPU sharding) */
    uint32_t flags;         /* SOCCER_F_* */
    uint32_t envs_per_thread; /* 0 = library default; 1, 4 or 8 force a vector width */
    void*    stream;        /* hipStream_t to enqueue on, or NULL: the handle creates its own */
} soccer_config;

/* batched_step_ex arguments.  Required: act_a, act_b (each unless that player has a fixed policy).
 * Every output may be NULL (skipped).
 * Action bytes: 0..4.  The *_host / *_staged entry points check every byte on the CPU and return
 * SOCCER_E_INVALID for anything else (nothing is launched).  On the device-pointer paths (batched_step,
 * batched_step_ex, batched_rollout) the kernels cannot raise: a byte b executes as the move table[b & 7] with
 * 5..7 = NOOP — so no value can index outside a rule table or leave the pitch — and any byte outside 0..4 sets
 * the sticky SOCCER_MISUSE_ACTION flag (soccer_get_stats / soccer_peek_misuse). */
typedef struct soccer_step_args {
    const int8_t*  act_a;       /* [n] action of player A, 0..4 */
    const int8_t*  act_b;       /* [n] action of player B, 0..4 */
    const double*  u_step;      /* [n] uniforms for outcome selection, or NULL: per-lane Philox */
    const double*  u_reset;     /* [n] uniforms for in-step auto-reset, or NULL: per-lane Philox */
    uint16_t*      obs;         /* [n] observation index after the step (after auto-reset if it fired) */
    int8_t*        reward;      /* [n] player A's reward -1/0/+1; B's is the negation (:400-402) */
    uint8_t*       terminated;  /* [n] done flag of the sampled transition (:403) */
    uint8_t*       truncated;   /* [n] timestep >= max_steps (:404) */
    uint8_t*       prob_code;   /* [n] code of the sampled transition's probability, see soccer_prob_table */
    uint16_t*      final_obs;   /* [n] observation BEFORE auto-reset (equals obs when none fired) */
    int8_t*        last_return; /* [n] A's return of the lane's most recently finished episode; written
                                   only on the step an episode ends (terminated or truncated) */
    /* ABI 2: what a gym-style caller reads every step, written by the same launch instead of by cast kernels of its own
     * (device pointers only; NULL = skipped) */
    float*         reward_a_f32; /* [n] player A's reward as float32 (-1.0 / 0.0 / +1.0), :400 */
    float*         reward_b_f32; /* [n] player B's reward as float32 = 0 - A's (:401-402); zeros are +0.0 */
    uint8_t*       finished;     /* [n] terminated | truncated (the vector env's infos["_final_observation"]) */
} soccer_step_args;

/* batched_rollout arguments: T fused steps with state held in registers.
 * Step j of the rollout is bit-identical to the j-th of T successive batched_step calls. */
typedef struct soccer_rollout_args {
    int32_t        n_steps;     /* T >= 1 */
    int32_t        sample_actions; /* 0: read act_a/act_b; 1: draw uniform-random actions in-kernel
                                      from the lane's word w of the purpose-1 Philox block, 15 bits per
                                      player: da = w & 0x7fff, db = (w >> 16) & 0x7fff;
                                      a = (da*5)>>15, b = (db*5)>>15 */
    const int8_t*  act_a;       /* [T][n] (row stride act_stride) or NULL when sample_actions */
    const int8_t*  act_b;
    int64_t        act_stride;  /* elements between consecutive steps (>= n) */
    uint16_t*      obs;         /* [T][n] trajectories (row stride out_stride) or NULL */
    int8_t*        reward;
    uint8_t*       terminated;
    uint8_t*       truncated;
    int64_t        out_stride;
    int32_t*       return_sum;  /* [n] += sum of A's rewards over the T steps, or NULL */
    int32_t*       episode_count; /* [n] += episodes finished during the T steps, or NULL */
    /* sample_actions only: mixed (stochastic) policies, DEVICE uint16[n_states][4].  Row s holds
     * floor(32768 * cumulative probability) of actions 0..3 at observation s (values 0..32768; action 4
     * takes the rest); the action is the number of thresholds <= the player's 15-bit draw.  NULL:
     * uniform.  This is the self-play rollout of BASELINE config 5. */
    const uint16_t* mix_a;
    const uint16_t* mix_b;
} soccer_rollout_args;

/* batched_rollout_ex: per-step trajectories beyond the four result streams — what gym's vector convention reports next to them
 * every step.  [T][n] with the args' out_stride; NULL = skipped.  With both NULL (or extra == NULL) the call IS batched_rollout. */
typedef struct soccer_rollout_extra {
    uint16_t*      final_obs;   /* observation BEFORE any auto-reset of that step (== obs where none fired); goal tuples -> 0 (:493-494) */
    uint8_t*       prob_code;   /* code of the sampled transition's probability, see soccer_prob_table (info['p'], :405) */
} soccer_rollout_extra;

/* ---- lifetime ------------------------------------------------------------------------- */
int soccer_abi_version(void);
int soccer_device_count(int* count);
/* replaces SoccerSimultaneousEnv.__init__ (:35-144): validates like its asserts (:45-46),
 * derives goal rows/cols (:60-61), classifies and numbers the state tuples (:63-109), builds the
 * ISD (:146-165) and the move/bounds table (:364-373), uploads them, allocates the SoA state.
 * Lanes start in the "needs reset" condition (:140). */
int soccer_create(const soccer_config* cfg, soccer_handle** out);
int soccer_destroy(soccer_handle* h);
const char* soccer_last_error(const soccer_handle* h);
/* np_random.seed(seed) (:411-412): re-key Philox and restart the tick counter at 0. */
int soccer_seed(soccer_handle* h, uint64_t seed);
int soccer_sync(soccer_handle* h);

/* ---- the hot path --------------------------------------------------------------------- */
/* reset (:410-424) for all lanes (mask NULL) or the lanes with mask[i] != 0.
 * u_reset NULL: the lane's Philox word.  obs (nullable) receives every lane's current observation. */
int batched_reset(soccer_handle* h, const uint8_t* mask, const double* u_reset, uint16_t* obs);
/* step (:375-408) for all lanes with per-lane Philox randomness. */
int batched_step(soccer_handle* h, const int8_t* act_a, const int8_t* act_b,
                 uint16_t* obs, int8_t* reward, uint8_t* terminated, uint8_t* truncated,
                 uint8_t* prob_code);
int batched_step_ex(soccer_handle* h, const soccer_step_args* args);
int batched_rollout(soccer_handle* h, const soccer_rollout_args* args);
int batched_rollout_ex(soccer_handle* h, const soccer_rollout_args* args, const soccer_rollout_extra* extra);

/* Host-pointer variants for small batches and numpy callers (the single-env facade): identical
 * semantics, but every array pointer is HOST memory.  The call stages inputs through one pinned
 * block (one copy in, one kernel, one copy out) and returns when the results are in the caller's
 * arrays.  last_return must be NULL. */
int batched_step_host(soccer_handle* h, const soccer_step_args* host_args);
int batched_reset_host(soccer_handle* h, const uint8_t* mask, const double* u_reset, uint16_t* obs);

/* Zero-copy form of the above: the caller fills the input arrays of the handle's pinned staging block
 * (soccer_staging gives their HOST addresses, n_lanes elements each, valid for the handle's lifetime),
 * calls batched_step_staged / batched_reset_staged with the SOCCER_STAGE_* bits of the inputs it filled,
 * and reads the results from the block's output arrays (overwritten by the next staged call). */
#define SOCCER_STAGE_ACT_A   1u
#define SOCCER_STAGE_ACT_B   2u
#define SOCCER_STAGE_U_STEP  4u
#define SOCCER_STAGE_U_RESET 8u
#define SOCCER_STAGE_MASK    16u
typedef struct soccer_staging_view {
    int8_t* act_a; int8_t* act_b; uint8_t* mask; double* u_step; double* u_reset;          /* inputs  */
    uint16_t* obs; uint16_t* final_obs; int8_t* reward; uint8_t* terminated; uint8_t* truncated;
    uint8_t* prob_code;                                                                      /* outputs */
} soccer_staging_view;
int soccer_staging(soccer_handle* h, soccer_staging_view* view);
int batched_step_staged(soccer_handle* h, uint32_t inputs);
int batched_reset_staged(soccer_handle* h, uint32_t inputs);

/* Single-agent mode (reference :54-56, :187-188, :266-279): `player` (0 = player_a, 1 = player_b) follows
 * a fixed policy — HOST int8[n_states], action per observation index — looked up with the observation
 * of the CURRENT tuple before every step; that player's action stream may then be NULL.  Only one
 * side may have a policy (:38).  policy NULL clears it.  Rewards stay player A's (+1 A scores); a
 * learner-B host negates them as the reference's table does (:243-244). */
int soccer_set_policy(soccer_handle* h, int32_t player, const int8_t* policy_host, int32_t n_states);

/* ---- one environment, lowest latency (the single-env facade; reference :375-424) --------- */
/* For handles with n_lanes == 1.  The current tuple, the actions and the uniform go in BY VALUE (kernel
 * arguments), the result comes back through a host-mapped record that the kernel writes with one 16-byte
 * store and the call polls: the GPU reads no host memory and the host enters no stream synchronisation
 * (~2x lower latency than batched_step_host on a mapped handle, tools/labs/latency_lab.hip).
 * soccer_step_scalar: in  = row_a..col_b, poss, t, act_a, act_b (ignored for a side with a fixed policy),
 *                           u_step, u_reset (used only with SOCCER_F_AUTORESET);
 *                     out = the next tuple / poss / t / needs_reset in the same fields, obs, reward (player A's),
 *                           terminated, truncated, prob_code.  needs_reset != 0 on input is the reference's
 *                           "Please reset the environment before taking a step" (SOCCER_E_INVALID, :376);
 *                           tuples outside the pitch or unreachable are SOCCER_E_INVALID.
 * soccer_reset_scalar: in = u_reset (the ISD draw, :414); out = tuple, poss, t = 0, obs.
 * Both consume one tick and leave the lane's resident state equal to the returned one.
 * The record: {seq, results, next tuple, flags | t << 8 | check << 16 | seq << 24} written by ONE global_store_dwordx4
 * to host-mapped memory.  The call accepts it only when word 0 == seq, the top byte of word 3 == seq's low byte AND
 * the check byte of word 3 equals the byte-sum of words 1 and 2 of the same call — so a record whose four dwords
 * did not all land (a torn 16-byte write; not observed on gfx950 / PCIe, but not an architectural promise) is
 * never taken for a complete one: the poll simply continues until they have. */
typedef struct soccer_scalar_io {
    int8_t row_a, col_a, row_b, col_b;
    uint8_t poss, needs_reset, t;
    int8_t act_a, act_b;
    int8_t reward;
    uint8_t terminated, truncated, prob_code;
    uint8_t pad_;
    uint16_t obs;
    double u_step, u_reset;
} soccer_scalar_io;
int soccer_step_scalar(soccer_handle* h, soccer_scalar_io* io);
int soccer_reset_scalar(soccer_handle* h, soccer_scalar_io* io);

/* SOCCER_F_HOST_MAPPED handles only: HOST address of the six state streams (row_a, col_a, row_b, col_b,
 * poss|needs_reset<<1, t; `stride` bytes apart).  Valid to read/write whenever the stream is idle
 * (after a *_host call or soccer_sync); writes bypass the tuple validation of soccer_set_state.
 * Only mapped handles are sure to have these six streams: how any other handle lays out its resident
 * state is private to the library (soccer_state_streams), reached through soccer_get_state / soccer_set_state. */
int soccer_host_view(soccer_handle* h, uint8_t** state, uint64_t* stride);

/* Number of byte streams the handle's resident state occupies: 3 (packed: possession, rows and columns of a
 * player share a byte; pitches of at most 8 rows and 16 columns incl. the goal columns, not host-mapped) or 6.
 * Results never depend on it.  The environment variable SOCCER_STATE_LAYOUT=wide, read by soccer_create,
 * forces 6 (tests and A/B runs).  0 for a NULL handle. */
int soccer_state_streams(const soccer_handle* h);

/* Which launch shape the handle's most recent batched_rollout / batched_rollout_ex call took (of a call longer than one
 * 4096-step chunk: its last chunk; every chunk of a call takes the same shape).  Read-only diagnostics for tests and A/B runs:
 * results never depend on any of it.  The host records it while it enqueues, so there is nothing to wait for.
 *   kernel          SOCCER_ROLLOUT_NONE before the first rollout (every other field is then 0 except lds_limit),
 *                   SOCCER_ROLLOUT_BYTE_PARALLEL (four lanes per thread; pitches and slips that fit the byte arithmetic) or
 *                   SOCCER_ROLLOUT_PER_LANE (through the rule tables)
 *   tail            1: the byte-parallel launch covered n_lanes & ~3 lanes and a per-lane launch on the same ticks the rest
 *   action_source   where the kernel takes the actions from.  Byte-parallel: 0 both action streams, 1 both sampled uniformly,
 *                   2 both sampled from mixed-policy tables held in LDS as one 16-byte row per state, 4 / 5 player A / B
 *                   follows its fixed policy and the other side is streamed, 3 anything else (a table on one side only,
 *                   tables beyond LDS, a fixed policy against a sampled side).  Per-lane: 0 both streams, 3 anything else
 *   slip_selection  byte-parallel: 0 slip_prob == 0, 1 thresholds compared one by one, 2 by the bucket table (16.5 KB of
 *                   static LDS).  Per-lane: 0 / 1 = slip_prob == 0 / > 0
 *   small_pitch, full   byte-parallel: the geometry form for small pitches; the form that also writes final_obs / prob_code.
 *                   Per-lane: 0, and whether the call asked for final_obs / prob_code
 *   table_placement where the observation-keyed tables (mixed-policy rows, fixed policies) are read from:
 *                   SOCCER_TABLES_NONE (the shape has none), SOCCER_TABLES_LDS (every workgroup stages them on entry) or
 *                   SOCCER_TABLES_GLOBAL.  Byte-parallel rule: they go to LDS when, next to the 144 B of slip rows, they fit
 *                   lds_limit minus the 16 KB + 16 B action staging area (only when an action stream is read) minus the
 *                   static bucket table (only with slip_selection 2) — 16 B per state when both sides are sampled from
 *                   tables, otherwise 2 x 8 B + 2 x 1 B (padded to 16) per state.  Per-lane: always global
 *   parts           byte-parallel launches per chunk (handles beyond 2^30 lanes are rolled out part by part; every part
 *                   stages its own tables); 1 for the per-lane kernel
 *   chunks          launches in time: ceil(n_steps / 4096)
 *   dynamic_lds_bytes   dynamic LDS of the (main) launch; above 48 KB the kernel's limit is raised first
 *   lds_limit       what a workgroup of this device may be given (64 KB on CDNA3, 160 KB on gfx950); set at create */
#define SOCCER_ROLLOUT_NONE          0
#define SOCCER_ROLLOUT_BYTE_PARALLEL 1
#define SOCCER_ROLLOUT_PER_LANE      2
#define SOCCER_TABLES_NONE   0
#define SOCCER_TABLES_LDS    1
#define SOCCER_TABLES_GLOBAL 2
typedef struct soccer_rollout_shape_info {
    int32_t  kernel, tail, action_source, slip_selection, small_pitch, full, table_placement, parts, chunks;
    int32_t  reserved_;
    uint64_t dynamic_lds_bytes;
    uint64_t lds_limit;
} soccer_rollout_shape_info;
int soccer_rollout_shape(const soccer_handle* h, soccer_rollout_shape_info* out);

/* ---- state injection / readback (`env.state = tuple`, tests/test_deterministic...py:43) -- */
/* HOST pointers of n_lanes elements; any pointer may be NULL (field left unchanged / not read).
 * These synchronise the stream. */
int soccer_set_state(soccer_handle* h, const int8_t* row_a, const int8_t* col_a,
                     const int8_t* row_b, const int8_t* col_b, const uint8_t* poss,
                     const uint8_t* t, const uint8_t* needs_reset);
int soccer_get_state(soccer_handle* h, int8_t* row_a, int8_t* col_a, int8_t* row_b, int8_t* col_b,
                     uint8_t* poss, uint8_t* t, uint8_t* needs_reset);

/* ---- rule tables (what the reference exposes as state_space / goal_states / isd) --------- */
/* n_states = nS (:64,:105-106) incl. the terminal index 0; lut_len = H*(W+2)*H*(W+2)*2 */
int soccer_dims(const soccer_handle* h, int32_t* n_states, int32_t* lut_len,
                int32_t* n_isd, int32_t* internal_width);
/* HOST outputs. lut[(((ra*W+ca)*H+rb)*W+cb)*2+p] = observation index, 0 for goal tuples,
 * 0xFFFF for unreachable tuples (:73-88); goal_value = +1/-1 for goal tuples (:94-102), else 0;
 * isd_states[n_isd][5] (:146-165). Any pointer may be NULL. */
int soccer_get_tables(const soccer_handle* h, uint16_t* lut, int8_t* goal_value, int8_t* isd_states);
/* The reference's transition relation P_readable (:167-293), computed on the device by the same rule
 * functions the step kernels use.  HOST outputs, key = lut index * 25 + action_a * 5 + action_b:
 *   count[key]           entries in the list (1..36), -1 for unreachable tuples (the reference has no key)
 *   prob/next_flat/reward/done[key*36 + k]   k-th entry in the reference's list order: probability
 *   (float64, weight * outcome probability, :241), lut index of the next tuple, player A's reward,
 *   done (:235-240). */
int soccer_enumerate_transitions(soccer_handle* h, int32_t* count, double* prob, int32_t* next_flat,
                                 int8_t* reward, uint8_t* done);
/* ---- planners (reference gym_soccer/utils/planners.py) ---------------------------------- */
/* All of them need a single-agent handle (exactly one side has a policy: soccer_set_policy) and work on the
 * learner's tables P[s][a] / Pmat / Rmat exactly as the reference's constructor builds them (:167-293), here
 * assembled from soccer_enumerate_transitions and cached on the handle until the policy changes.  One
 * single-workgroup kernel runs a whole planner; float64 throughout.  Inputs and outputs are HOST arrays
 * (V[n_states], Q[n_states*5], pi[n_states] int32); any output may be NULL.  max_sweeps bounds the total
 * number of sweeps over the state space, over all evaluations of policy iteration and modified policy iteration, whose
 * greedy steps count as sweeps too.  A sweep that reaches it without meeting the stopping rule ends the call with
 * SOCCER_E_STATE, the counter is still written, and the outputs hold:
 *   value iteration             V the iterate the last sweep started from, Q and pi that sweep's (as when it converges)
 *   policy evaluation, dense evaluation   the last iterate computed.  Dense evaluation stops after k sweeps anyway; when the
 *                               k-th is also sweep max_sweeps and the change is still >= theta, it returns SOCCER_E_STATE too
 *   policy iteration            V the iterate at which the evaluation in progress was cut off, Q and pi one improvement
 *                               from that V, which is counted
 *   modified policy iteration   cut off at a greedy step: V = max_a Q, Q and pi of that step; inside an evaluation: V that
 *                               evaluation's last iterate, Q and pi of the greedy step it started from, the evaluation counted
 * The state count is bounded by the workgroup's LDS (V[n_states] in float64 must fit in 150 KiB: 14x7 is the largest 7-row
 * pitch, 13x8 is refused with SOCCER_E_INVALID "too many states").
 *
 * The list-based planners evaluate  Q[s][a] += prob * (reward + discount_factor * V[next] * (not done))  in
 * list order like the reference: values, greedy policies and iteration counts are the reference's BIT FOR BIT.
 *   soccer_value_iteration     planners.py:4-18   sweeps until max|V - max_a Q| < theta; V is the pre-update
 *                                                 iterate (as the reference returns it), pi the first argmax
 *   soccer_policy_evaluation   planners.py:20-31  V of the deterministic policy pi, from zeros
 *   soccer_policy_improvement  planners.py:33-41  Q from V, new_pi = first argmax
 *   soccer_policy_iteration    planners.py:43-53  from pi0 (the reference draws it with np.random.choice) until
 *                                                 the greedy policy stops changing; V belongs to the last evaluation
 * The dense planners follow the reference's Pmat/Rmat algebra (r + discount_factor * Pmat @ v) with a sequential
 * dot; numpy's BLAS dot associates differently, so they agree with the reference to rounding (~1e-15 relative):
 *   soccer_policy_eval_dense            planners.py:55-70  at most k sweeps of a stochastic policy[n_states*5]
 *                                                          from init (NULL = zeros), stops when the change < theta
 *   soccer_modified_policy_iteration    planners.py:73-87  greedy step + k evaluation sweeps, stops when
 *                                                          |v - greedy_v| <= theta*(1-discount)/(2*discount); V = greedy_v */
int soccer_value_iteration(soccer_handle* h, double theta, double discount_factor, int32_t max_sweeps,
                           double* V, double* Q, int32_t* pi, int32_t* iterations);
int soccer_policy_evaluation(soccer_handle* h, const int32_t* pi, double theta, double discount_factor,
                             int32_t max_sweeps, double* V, int32_t* sweeps);
int soccer_policy_improvement(soccer_handle* h, const double* V, double discount_factor, double* Q, int32_t* new_pi);
int soccer_policy_iteration(soccer_handle* h, const int32_t* pi0, double theta, double discount_factor,
                            int32_t max_sweeps, double* V, double* Q, int32_t* pi, int32_t* iterations);
int soccer_policy_eval_dense(soccer_handle* h, const double* policy, int32_t k, double theta, double discount_factor,
                             int32_t max_sweeps, const double* init, double* v, int32_t* sweeps);
int soccer_modified_policy_iteration(soccer_handle* h, int32_t k, double theta, double discount_factor,
                                     int32_t max_sweeps, double* V, double* Q, int32_t* pi, int32_t* iterations);
/* ---- minimax planners (two-player handles; Shapley's value iteration, Littman 1994) ---------------------------
 * A 5x5 zero-sum stage game is solved in float64 by csrc/soccer_games.hpp: a pure saddle point exactly (first row
 * whose minimum is the max-min, first column whose maximum is the min-max), otherwise the simplex method with Bland's
 * rule, whose answer is verified against the bracket its strategies certify and, where that is wider than eps, replaced
 * by the first Shapley-Snow square-submatrix candidate that passes.  With eps = 1e-10 * max(1, max|A|) the result
 * satisfies  min_b (x^T A)_b >= v - eps,  max_a (A y)_a <= v + eps,  x, y >= 0,  sum x = sum y = 1 within 1e-12
 * (the strategies certify a bracket at most eps wide and v is its midpoint).  The same input gives the same bits.
 * Inputs and outputs are HOST arrays; any output may be NULL.  None of these calls consumes a tick or touches the
 * lanes' state; during a graph capture they return SOCCER_E_STATE. */
/* n games of 5x5, A[g][a][b] = row player's (A's) payoff -> value[n], maximin x[n][5] of A, minimax y[n][5] of B */
int soccer_solve_matrix_games(soccer_handle* h, int64_t n_games, const double* A,
                              double* value, double* x, double* y);
/* The planners need a two-player handle (SOCCER_E_INVALID with a fixed policy).  The (state, joint action) lists are
 * the two-player P[s][(a, b)] of the reference's constructor (player A's reward), assembled from
 * soccer_enumerate_transitions and cached on the handle.  Q[s][a][b] = sum_k prob * (reward + (discount_factor *
 * V[next]) * (not done)) in list order — bit for bit the host sum over P[s][(a, b)] — and V'[s] = val(Q[s]).
 * One Shapley operator application from the caller's V[n_states]: V_out = val(Q(V)), Q[n_states][5][5], the
 * stage-game strategies pi_a / pi_b [n_states][5]. */
int soccer_minimax_backup(soccer_handle* h, double discount_factor, const double* V,
                          double* V_out, double* Q, double* pi_a, double* pi_b);
/* V_0 = 0; sweep k: Q_k = Q(V_{k-1}), V_k = val(Q_k); stops at the first k with max|V_k - V_{k-1}| < theta.
 * Returns V_k, Q_k, the strategies of Q_k and k: (V, Q, pi) is self-consistent, V[s] = val(Q[s]).
 * (soccer_value_iteration returns the pre-update V, as the reference does; this one does not.)  SOCCER_E_STATE when
 * max_sweeps is reached; the outputs then hold the last iterate. */
int soccer_minimax_value_iteration(soccer_handle* h, double theta, double discount_factor, int32_t max_sweeps,
                                   double* V, double* Q, double* pi_a, double* pi_b, int32_t* iterations);
/* ---- best responses to mixed policies, and their exploitability (two-player handles) ---------------------------------
 * How badly can the best possible opponent beat a mixed policy?  n policies are solved in ONE sequence of launches, a
 * sweep over all (policy, state) pairs each.  With Q_k[s][a][b] the expression above over V_{k-1} (V_0 = 0, player A's
 * reward) and every sum below a sequential float64 sum from 0.0 in index order, acc = acc + p[i] * q[i], not contracted:
 *   response by B to A's mixed policy x (player = 0, the side that is held fixed):
 *       Qr_k[s][b] = sum_a x[s][a] * Q_k[s][a][b],   V_k[s] = min_b Qr_k[s][b],   br[s] = the first b that attains it
 *   response by A to B's mixed policy y (player = 1):
 *       Qr_k[s][a] = sum_b y[s][b] * Q_k[s][a][b],   V_k[s] = max_a Qr_k[s][a],   br[s] = the first a that attains it
 *   evaluation of a pair (x, y):
 *       V_k[s] = sum_a x[s][a] * (sum_b y[s][b] * Q_k[s][a][b])
 * Every mode stops at the first k with max_s |V_k[s] - V_{k-1}[s]| < theta and returns V_k, the Qr_k and br that belong
 * to it and k — a self-consistent triple, as soccer_minimax_value_iteration's is.  V is always player A's value: the
 * response to x is x's worst case, a lower bound on the game's value, the response to y an upper bound, and
 * (response to y) - (response to x) >= 0 is the exploitability of the pair.
 * Row 0 of a policy (the terminal observation) is not read: it counts as zeros, so V[0] = 0, Qr[0] = 0 and br[0] = 0.
 * Every other row must be >= 0 and sum to 1 as soccer_minimax_q_config::opponent_policy must (SOCCER_E_INVALID, the
 * message names policy and state); n is 1 .. SOCCER_BR_MAX_POLICIES, discount_factor in [0, 1], theta >= 0,
 * max_sweeps >= 1.  policy / pi_a / pi_b are HOST [n][n_states][5]; the outputs are HOST V[n][n_states],
 * Qr[n][n_states][5], br[n][n_states], iterations[n], and any of them may be NULL.
 * Batches: policy i returns exactly the bits it returns when it is solved alone.  Each has its own stopping sweep k_i
 * (iterations[i]); once it has converged its V, Qr and br stay those of sweep k_i while the others continue.
 * SOCCER_E_STATE when some policy has not converged after max_sweeps: iterations[i] = max_sweeps for those, whose outputs
 * hold the last iterate, and the others' results are complete.  Like the minimax planners these calls consume no tick,
 * leave the lanes alone and return SOCCER_E_STATE during a graph capture. */
#define SOCCER_BR_MAX_POLICIES 256
int soccer_best_response(soccer_handle* h, int32_t player, int32_t n_policies, const double* policy,
                         double theta, double discount_factor, int32_t max_sweeps,
                         double* V, double* Qr, int32_t* br, int32_t* iterations);
int soccer_evaluate_policies(soccer_handle* h, int32_t n_pairs, const double* pi_a, const double* pi_b,
                             double theta, double discount_factor, int32_t max_sweeps, double* V, int32_t* iterations);
/* ---- cross-play: the payoff matrix of n_a x n_b mixed policies (two-player handles) -----------------------------------
 * What does policy i of player A score against policy j of player B, for all i and j?  Pair (i, j) is exactly
 * soccer_evaluate_policies on (pi_a[i], pi_b[j]) solved alone: V_0 = 0, the same sequential float64 sums in the same
 * order, its own stopping sweep k_ij — V[i][j] and iterations[i][j] are the bits and the count that call returns.
 * payoff[i][j] is player A's value at kick-off: the sum of V[i][j][obs] over the handle's initial states in ISD order,
 * from 0.0, divided by n_isd (soccer_dims, soccer_get_tables).
 * pi_a is HOST [n_a][n_states][5], pi_b HOST [n_b][n_states][5]; payoff and iterations are HOST [n_a][n_b], V is HOST
 * [n_a][n_b][n_states]; any of the three may be NULL, and only what is asked for is formed and copied.  Row 0 of a policy
 * is not read and counts as zeros; the row check is soccer_evaluate_policies' on the n_a + n_b policies.  n_a and n_b are
 * 1 .. SOCCER_CROSS_MAX_POLICIES, discount_factor in [0, 1], theta >= 0, max_sweeps >= 1.  The policies are uploaded once
 * per call, (n_a + n_b) * n_states * 40 bytes, and nothing per pair.
 * pairs_per_pass is the number of pairs solved together on the device: 0 lets the library choose (as many as keep the two
 * V buffers of a pass, 2 * n_states * pairs * 8 bytes, at or under 1 GiB), otherwise a positive multiple of 64
 * (SOCCER_E_INVALID if not).  A matrix with more pairs is solved pass after pass; no result depends on this value.
 * SOCCER_E_STATE when some pair has not converged after max_sweeps: iterations == max_sweeps marks those, whose outputs
 * hold the last iterate, and the other pairs are complete.  Like the calls above this one consumes no tick, leaves the
 * lanes alone and returns SOCCER_E_STATE during a graph capture. */
#define SOCCER_CROSS_MAX_POLICIES 1024
int soccer_cross_play(soccer_handle* h, int32_t n_a, const double* pi_a, int32_t n_b, const double* pi_b,
                      double theta, double discount_factor, int32_t max_sweeps, int32_t pairs_per_pass,
                      double* payoff, double* V, int32_t* iterations);
/* ---- match outcomes: who wins, how often it is a draw, how long a game lasts (two-player handles) -----------------------
 * Littman's columns for every pair (x = pi_a[i], y = pi_b[j]): after every step the game goes on with probability
 * continue_prob = c in [0, 1] and is called a draw otherwise.  Three value vectors per pair, all 0 before sweep 1:
 *   W_A[n_states]  the probability that A's side is credited with the goal that ends the game
 *   W_B[n_states]  the same for B
 *   L[n_states]    the expected number of steps the game lasts
 * Sweep k, for every state s and joint action (a, b), over the list in list order, each sum acc = acc + .. from 0.0 in
 * float64, not contracted (the expression of Q above with three rewards):
 *   qA = sum prob * ((reward > 0 ? 1.0 : 0.0) + (c * W_A[next]) * (not done))
 *   qB = sum prob * ((reward < 0 ? 1.0 : 0.0) + (c * W_B[next]) * (not done))
 *   qL = sum prob * (1.0                      + (c * L  [next]) * (not done))
 * then each channel is mixed as soccer_evaluate_policies mixes Q: F_k[s] = sum_a x[s][a] * (sum_b y[s][b] * q[a][b]).
 * Padding entries are accumulated like any other.  Row 0 of a policy is not read and counts as zeros, so all three
 * channels are 0 at state 0.  (The lists' rewards are -1, 0 or +1 and nonzero only on entries that end the game.)
 * A pair stops at its first sweep k where the maximum over the three channels and all states of |F_k - F_{k-1}| is
 * < theta and keeps that sweep's vectors.  win_a, win_b and length are the kick-off numbers of W_A, W_B and L: the
 * sequential sum over the handle's initial states in ISD order, from 0.0, divided by n_isd, as soccer_cross_play's payoff.
 * The share of draws is 1 - win_a - win_b, and with c the discount, W_A - W_B is soccer_cross_play's V up to the stopping
 * error of three fixed points.  Every pair returns the bits and the sweep count it has when it is solved alone.
 * win_a, win_b, length and iterations are HOST [n_a][n_b], values is HOST [n_a][n_b][3][n_states] (W_A, W_B, L); any of
 * them may be NULL, and only what is asked for is formed and copied.  The checks, refusals, limits
 * (SOCCER_CROSS_MAX_POLICIES) and pairs_per_pass are soccer_cross_play's, the default pass keeping the two three-channel
 * buffers, 2 * 3 * n_states * pairs * 8 bytes, at or under 1 GiB.  continue_prob == 1 is allowed, as discount_factor == 1
 * is: L then grows by one per sweep wherever the pair never scores, and such pairs need not converge.
 * SOCCER_E_STATE when some pair has not converged after max_sweeps: iterations == max_sweeps marks those, whose outputs
 * hold the last iterate (the max_sweeps-step probabilities and the length truncated there), and the other pairs are
 * complete.  Like the calls above this one consumes no tick, leaves the lanes alone and returns SOCCER_E_STATE during a
 * graph capture. */
int soccer_match_outcomes(soccer_handle* h, int32_t n_a, const double* pi_a, int32_t n_b, const double* pi_b,
                          double theta, double continue_prob, int32_t max_sweeps, int32_t pairs_per_pass,
                          double* win_a, double* win_b, double* length, double* values, int32_t* iterations);
/* ---- state occupancy: where a game is played (two-player handles) -------------------------------------------------------
 * The occupancy measure of every pair (x = pi_a[i], y = pi_b[j]): D[s] is the expected number of visits to state s from
 * kick-off when after every step the game goes on with probability continue_prob = c in [0, 1], as in
 * soccer_match_outcomes — the dual of the value, computed forwards from the start instead of backwards from the goals.
 * The start distribution: mu[s] = 1.0 / (double)n_isd at each of the handle's initial observation indices (they are
 * distinct), 0.0 elsewhere.  D_0 = 0.  Sweep k, for every state s':
 *   acc = 0.0
 *   for every in-entry e of s', in in-list order:
 *       acc = acc + e.prob * ((x[s][a] * y[s][b]) * (c * D_{k-1}[s]))          with (s, a, b) e's source key
 *   D_k[s'] = mu[s'] + acc
 * in float64, nothing contracted: every product and sum is its own rounding, in exactly this association.
 * The in-list of s' holds every entry of the two-player lists (the lists of Q above, by state and joint action a * 5 + b)
 * whose next is s', whose done bit is clear and whose source state is not 0, ordered by ascending source key
 * s * 25 + a * 5 + b, then by position inside that key's list; padding entries of those lists are dropped.  Each in-list
 * is padded to a multiple of 4 entries with (prob 0.0, source key 0), which adds an exact +0.0.  Row 0 of a policy is not
 * read and counts as zeros, and D[0] is 0.0 in every sweep.
 * A pair stops at its first sweep k where max over s of |D_k[s] - D_{k-1}[s]| < theta and keeps that sweep's vector; every
 * pair returns the bits and the sweep count it has when it is solved alone.  For c < 1 this always happens (sweep k moves
 * no state by more than c^(k-1)); c == 1 is allowed and need not converge.
 *   length[n_a][n_b]            sum over s of D[s], sequential over ascending s from 0.0: the expected number of steps
 *   expect[n_a][n_b][n_f]       sum over s of D[s] * features[q][s], in the same order; features is HOST [n_f][n_states],
 *                               n_f is 0 .. SOCCER_OCC_MAX_FEATURES (an indicator gives the steps spent in a set of states)
 *   occupancy[n_a][n_b][n_states]
 *   iterations[n_a][n_b]
 * are HOST arrays; any of them may be NULL, and only what is asked for is formed and copied (features is not read when
 * expect is NULL).  sum D equals soccer_match_outcomes' length, and sum D * (the pair's expected reward per state) equals
 * soccer_cross_play's payoff with c the discount, each up to the stopping errors.  The checks, refusals, limits
 * (SOCCER_CROSS_MAX_POLICIES) and pairs_per_pass are soccer_cross_play's, the default pass keeping the two D buffers,
 * 2 * n_states * pairs * 8 bytes, at or under 1 GiB.  SOCCER_E_STATE when some pair has not converged after max_sweeps:
 * iterations == max_sweeps marks those, whose outputs hold the last iterate, and the other pairs are complete.  Like the
 * calls above this one consumes no tick, leaves the lanes alone and returns SOCCER_E_STATE during a graph capture. */
#define SOCCER_OCC_MAX_FEATURES 16
int soccer_occupancy(soccer_handle* h, int32_t n_a, const double* pi_a, int32_t n_b, const double* pi_b,
                     double theta, double continue_prob, int32_t max_sweeps, int32_t pairs_per_pass,
                     int32_t n_f, const double* features,
                     double* length, double* expect, double* occupancy, int32_t* iterations);
/* ---- exact policy gradients of policy pairs, and gradient play on them (two-player handles) -----------------------------
 * Under the direct parametrisation, with gamma = discount_factor and D the gamma-discounted occupancy from kick-off,
 *   d payoff(x, y) / d x[s][a] = D[s] * Q_a[s][a],   Q_a[s][a] = sum_b y[s][b] * Q[s][a][b]
 * and player B's has the same form with Q_b[s][b] = sum_a x[s][a] * Q[s][a][b].  All arithmetic is float64, nothing is
 * contracted, and every product and sum is its own rounding in the association written.
 * Per pair (i, j), with x = pi_a[i] and y = pi_b[j]:
 *   V is exactly soccer_cross_play's vector for the pair: V_0 = 0, with its own stopping sweep k_V.
 *   D is exactly soccer_occupancy's vector with continue_prob = discount_factor, with its own stopping sweep k_D.
 *   One more backup from the pair's final V follows: q[a][b] is the list sum of "Q above", which is the expression of
 *   soccer_minimax_value_iteration's Q with padding entries accumulated.
 *   Q_a[s][a] = sum_b y[s][b] * q[a][b], for b = 0..4 from 0.0.
 *   Q_b[s][b] = sum_a x[s][a] * q[a][b], for a = 0..4 from 0.0.
 *   Row 0 of a policy counts as zeros, so both are 0 at state 0.
 *   payoff is cross-play's kick-off mean of V.
 * Per policy:
 *   Weights: w_b is HOST [n_b], w_a is HOST [n_a].  NULL means every weight is 1.0 / (double)n.
 *   reach_a[i][s] = sum_j w_b[j] * D_ij[s], sequential over ascending j from 0.0.
 *   grad_a[i][s][a] = sum_j w_b[j] * (D_ij[s] * Q_a,ij[s][a]), in the same order.
 *   reach_b[j][s] and grad_b[j][s][b] sum over ascending i with w_a[i].
 *   With normalize != 0: grad_a[i][s][a] = reach_a[i][s] > 0.0 ? grad_a[i][s][a] / reach_a[i][s] : 0.0, and likewise for B.
 *   grad_b is the gradient of player A's payoff, so B descends it.
 * grad_a[i] is the exact gradient of sum_j w_b[j] * payoff(pi_a[i], pi_b[j]), player A's payoff against a kick-off mixture
 * of opponents (up to the stopping errors of the solves), which no Markov policy of the opponent reproduces.
 * Outputs, all HOST arrays; any may be NULL, and only what is asked for is formed and copied:
 *   payoff[n_a][n_b]   grad_a[n_a][n_states][5]   grad_b[n_b][n_states][5]   reach_a[n_a][n_states]   reach_b[n_b][n_states]
 *   q_a, q_b [n_a][n_b][n_states][5]   V, occupancy [n_a][n_b][n_states]   iterations[n_a][n_b][2] holding (k_V, k_D)
 * The checks, limits (SOCCER_CROSS_MAX_POLICIES), pairs_per_pass and refusals are soccer_cross_play's.  Weights must be
 * finite, >= 0 and not all zero.  The default pass keeps this call's buffers at or under 1 GiB: two V, two D and the ten
 * action-value planes, 14 * n_states * pairs * 8 bytes.  SOCCER_E_STATE when some pair has an open V or D solve after
 * max_sweeps: those pairs hold the last iterates, and what was formed from them (iterations == max_sweeps marks the open
 * solve).  Every pair and every policy returns the bits it has when solved alone: no result depends on the passes, on
 * earlier calls or on which outputs are asked for.  A row or column of the matrix that spans passes keeps the one sequential
 * order: the running sums are carried from pass to pass.  Like the calls above this one consumes no tick, leaves the lanes
 * alone and returns SOCCER_E_STATE during a graph capture. */
int soccer_policy_gradient(soccer_handle* h, int32_t n_a, const double* pi_a, int32_t n_b, const double* pi_b,
                           double theta, double discount_factor, int32_t max_sweeps, int32_t pairs_per_pass,
                           const double* w_a, const double* w_b, int32_t normalize,
                           double* payoff, double* grad_a, double* grad_b, double* reach_a, double* reach_b,
                           double* q_a, double* q_b, double* V, double* occupancy, int32_t* iterations);
/* Gradient play: n_a policies of player A and n_b of player B live on the device and take projected gradient steps against
 * each other's weighted mixture.  Resident state: x[n_a][n_states][5], y[n_b][n_states][5], the previous step's gradients
 * prev_a and prev_b, steps, the weights (uniform until soccer_gradient_play_set_weights; NULL there is uniform again) and the
 * last completed step's payoff matrix.  One step of soccer_gradient_play_run:
 *   g_a and g_b are exactly soccer_policy_gradient's grad_a and grad_b on the resident policies, with the resident weights
 *   and the config's normalize, discount_factor, theta, max_sweeps and pairs_per_pass; no policy leaves the device.
 *   At steps == 0, prev = g.  The direction is d = g + optimism * (g - prev).  Then prev = g.
 *   For every s >= 1: x[s] = P(x[s][a] + eta_a * d_a[s][a]) and y[s] = P(y[s][b] - eta_b * d_b[s][b]).  Row 0 is never touched.
 *   A side whose eta is 0.0 is held fixed: none of its rows is written (P of a row whose sum is not exactly 1.0 would move it
 *   by ulps), only its prev follows g.
 * P is the projection onto the simplex of five: u is v sorted in descending order; css is the running sum of u from 0.0;
 * for k = 1..5, t = (css_k - 1.0) / (double)k, and tau = t at k = 1 and whenever u_k - t > 0.0; out[a] = v[a] - tau where that
 * is > 0.0, else 0.0 (csrc/soccer_simplex.hpp, a plain header a host program can run).
 * trace is HOST [n_steps][n_a][n_b] or NULL: each completed step's payoff matrix before its update.  A step whose solves are
 * still open at max_sweeps is not applied: run returns SOCCER_E_STATE, and steps counts the completed steps.
 * The config: n_a, n_b as soccer_policy_gradient's; eta_a, eta_b finite and >= 0; optimism in [0, 1]; pi_a / pi_b HOST
 * [n][n_states][5] checked like soccer_cross_play's, NULL means uniform.  run(T) leaves the bits that T rounds of
 * soccer_policy_gradient on what _read returns, followed by the update above, leave.  A learner is owned by the handle and
 * freed with it; its calls consume no tick and return SOCCER_E_STATE during a graph capture.  _read: any output may be NULL;
 * _load: NULL leaves that part as it is, and the policies are checked like the config's; with everything _read returns but
 * the weights, a fresh learner continues bit for bit. */
typedef struct soccer_gradient_play soccer_gradient_play;
typedef struct soccer_gradient_play_config {
    int32_t n_a, n_b;
    double eta_a, eta_b, optimism;
    double discount_factor, theta;
    int32_t normalize, max_sweeps, pairs_per_pass, reserved_;
    const double* pi_a;
    const double* pi_b;
} soccer_gradient_play_config;
int soccer_gradient_play_create(soccer_handle* h, const soccer_gradient_play_config* cfg, soccer_gradient_play** out);
int soccer_gradient_play_destroy(soccer_handle* h, soccer_gradient_play* g);
int soccer_gradient_play_run(soccer_handle* h, soccer_gradient_play* g, int32_t n_steps, double* trace);
int soccer_gradient_play_read(soccer_handle* h, soccer_gradient_play* g, double* pi_a, double* pi_b, double* prev_a, double* prev_b,
                              double* w_a, double* w_b, double* payoff, int64_t* steps);
int soccer_gradient_play_load(soccer_handle* h, soccer_gradient_play* g, const double* pi_a, const double* pi_b,
                              const double* prev_a, const double* prev_b, const double* payoff, const int64_t* steps);
int soccer_gradient_play_set_weights(soccer_handle* h, soccer_gradient_play* g, const double* w_a, const double* w_b);
/* ---- the meta-game: maximin mixtures of n_a x n_b zero-sum matrix games (any handle) ------------------------------------
 * Which mixture of the rows of a payoff matrix (soccer_cross_play's, or any other) can a rational opponent not beat?
 * A is HOST [n_games][n_a][n_b], the row player's (the maximiser's) payoffs.  Per game, in float64, nothing contracted
 * (a product and the sum that takes it are two roundings), every reduction with an index tie-break, so that no bit
 * depends on how the work is spread over threads:
 *  1. Saddle point.  rmin[i] = min_j A[i][j], cmax[j] = max_i A[i][j].  If max_i rmin == min_j cmax: i* is the first row
 *     attaining it, j* the first column, x = e_i*, y = e_j*, value = lo = hi = A[i*][j*] bit for bit, status 1, 0 pivots.
 *  2. Tableau.  lo_A = min A, range = max A - lo_A (> 0 here).  n_a + 1 rows, n_b + n_a + 2 columns: the structural
 *     columns T[i][j] = (A[i][j] - lo_A) / range + 1.0, the slack identity, the right-hand side R = 1.0, and a SHADOW
 *     right-hand side S[i] = 1.0 + (i + 1) * 2^-26 (exact); the objective row is -1.0 under the structural columns and
 *     0.0 elsewhere; basis[i] = n_b + i.
 *  3. Pivot.  c = the column among the first n_a + n_b with the smallest objective entry, lowest index on ties
 *     (Dantzig); the game is finished unless that entry is < -1e-12; if pivots == max_pivots, stop with status 3; r =
 *     among the rows with T[i][c] > 1e-12 the one with the smallest T[i][R] / T[i][c], ties (equal quotients) to the
 *     smallest T[i][S] / T[i][c], then to the lowest i (no such row: impossible for a positive matrix, kept as a guard:
 *     stop with status 3).  row' = T[r][.] / T[r][c] with row'[c] =
 *     1.0; every other row, the objective included, becomes T[i][j] - T[i][c] * row'[j] over all columns, R and S too,
 *     with T[i][c] = 0.0 afterwards — no row is skipped because its factor is 0, which fixes the signs of zeros;
 *     basis[r] = c.
 *  4. Strategies.  y[j] = max(T[r][R], 0) where basis[r] == j, else 0; x[i] = max(T[objective][n_b + i], 0); each divided
 *     by its sequential sum in index order from 0.0; a sum that is not positive gives the uniform strategy.
 *  5. Bracket, on the caller's A.  lo = min_j sum_i x[i] * A[i][j], hi = max_i sum_j A[i][j] * y[j], the sums sequential
 *     from 0.0 in index order (acc = acc + p * q); value = 0.5 * (lo + hi); with eps = 1e-10 * max(1, max|A|) a finished
 *     game has status 0 when hi - lo <= eps, else status 2.
 * The shadow column only breaks the ratio test's ties (all-ones right-hand sides with tied or duplicated policies are
 * heavily degenerate): the quotients of the true column R come first, because a ratio test on the shadow column alone
 * lets entries of R go negative by the size of the perturbation, and the clipped strategies then certify a bracket that
 * wide.  The strategies are read from R.  The rule is no proof against cycling: max_pivots and status 3 are.  The contract is the certificate: lo <= the game's value <= hi holds for whatever x and y come out (a
 * tableau updated tens of thousands of times drifts: there is no reinversion), and the status says whether the bracket is
 * as narrow as eps.
 * n_a and n_b are 1 .. SOCCER_META_MAX_POLICIES, n_games >= 0 (0 returns SOCCER_OK at once), max_pivots >= 1.  A NaN or
 * infinite entry is SOCCER_E_INVALID, found on the host before anything is uploaded; the message names the game, the row
 * and the column.  A game whose max A - min A is not finite (finite entries further apart than DBL_MAX, such as 1e308 and
 * -1e308: step 2 would divide by it) is SOCCER_E_INVALID as well, saddle point or not, found in the same loop; the
 * message names the game.  Entries of +-8e307 are accepted.  path: 0 the library chooses, 1 the LDS kernel (a workgroup per game, the tableau in LDS, one launch;
 * SOCCER_E_INVALID "does not fit" unless 128 + 8 * ((n_a + 2) * stride + n_a + 1) + 4 * n_a bytes, stride = (n_a + n_b + 2)
 * rounded up to an odd number, are at most the LDS a workgroup may be given: 163 840 bytes on gfx950, so 99 x 99 fits
 * and 100 x 100 does not), 2 the global kernels (the tableaux in device memory, two launches per pivot).
 * pivots_per_sync >= 0: how many pivots the global path enqueues before it reads back how many games are still open (0:
 * the library chooses).  Games are solved in passes whose matrices and tableaux stay at or under 1 GiB.  Game g of a
 * batch returns the bits it returns alone, and no result depends on path or pivots_per_sync.
 * SOCCER_E_STATE when some game stopped at max_pivots (status 3): its outputs hold the strategies of the last basis and
 * their (valid) bracket, and the other games are complete.  Like soccer_solve_matrix_games the call has nothing to do with
 * the pitch: any handle will do, it consumes no tick, leaves the lanes alone and returns SOCCER_E_STATE during a graph
 * capture.  A NULL `out` asks for nothing. */
#define SOCCER_META_MAX_POLICIES 1024
typedef struct soccer_meta_game_result {   /* HOST pointers, any may be NULL */
    double*  value;    /* [n_games]            midpoint of the bracket */
    double*  x;        /* [n_games][n_a]       row player's (the maximiser's) mixture */
    double*  y;        /* [n_games][n_b]       column player's mixture */
    double*  lo;       /* [n_games]            min_j (x^T A)_j : what x guarantees */
    double*  hi;       /* [n_games]            max_i (A y)_i   : what y concedes at most */
    int32_t* pivots;   /* [n_games] */
    int32_t* status;   /* [n_games]  1 saddle point, 0 finished and hi - lo <= eps, 2 finished but wider, 3 stopped at max_pivots */
} soccer_meta_game_result;
int soccer_solve_meta_games(soccer_handle* h, int64_t n_games, int32_t n_a, int32_t n_b, const double* A /* HOST [n_games][n_a][n_b] */,
                            int32_t max_pivots, int32_t path, int32_t pivots_per_sync, const soccer_meta_game_result* out);
/* ---- learners (two-player handles; minimax-Q, Littman 1994) ------------------------------------------------------
 * A learner lives on a two-player SOCCER_F_AUTORESET handle of at most 2^22 lanes and keeps ONE shared table
 * Q[n_states][5][5] (float64) on the device, with V[n_states] = val(Q[s]) and the stage-game strategies
 * pi_a / pi_b [n_states][5] (csrc/soccer_games.hpp), visits[n_states][25] (uint64), the learning rate alpha and a step
 * counter.  The handle's lanes are its actors.  One learner step, in this order:
 *   1. behaviour policies: player A draws from p = (1.0 - explor) * pi_a[s] + explor / 5.0, turned into the uint16[4]
 *      threshold row of soccer_rollout_args::mix_a (sequential float64 cumulative sum c, floor(c * 32768.0 + 1e-9),
 *      clipped to 0..32768); player B uniformly (SOCCER_MQ_UNIFORM), by the same expression on pi_b (SOCCER_MQ_SELF)
 *      or from the thresholds of a fixed mixed policy (SOCCER_MQ_FIXED, computed once)
 *   2. act and step: for the environment the step IS batched_rollout(n_steps = 1, sample_actions = 1, mix_a, mix_b) —
 *      same tick, same Philox words, same action draw, same auto-reset, same episode histogram, same misuse flags.  A
 *      lane yields s (its observation before the step), a, b, r (player A's reward), terminated and s' = final_obs
 *   3. reduce: with Vq[s] = rint(V[s] * 2^40) as int64, cell = s * 25 + a * 5 + b:  c[cell] += 1, R[cell] += r,
 *      SV[cell] += terminated ? 0 : Vq[s']  — INTEGER sums, so the result does not depend on the order in which lanes
 *      arrive (|V| <= 1 and at most 2^22 samples: the sums fit int64; the grid costs < 5e-13 per sample)
 *   4. update, for every cell with c > 0:  m = ((double)R + discount_factor * ((double)SV * 2^-40)) / (double)c,
 *      Q = Q + alpha * (m - Q),  visits += c
 *   5. re-solve: (V[s], pi_a[s], pi_b[s]) = solve(Q[s]) for every state with a touched cell
 *   6. alpha = alpha * decay, steps += 1
 * Initially Q[s] = V[s] = q_init and pi_a[s] = pi_b[s] = 0.2 for every live s (set, not solved), Q[0] = V[0] = 0 (index
 * 0 is the terminal observation and never a current state), visits = 0.  With alpha, q_init and the rewards in range
 * every Q and V stays in [-1, 1].  The learner's state is a fixed function of (seed, parameters, number of steps): it
 * does not depend on launch geometry, vector width or state layout.  Lanes that still need their first reset are left
 * untouched (SOCCER_MISUSE_FROZEN) and contribute nothing.
 * Errors: a handle with a fixed policy, without SOCCER_F_AUTORESET or with more than 2^22 lanes, and parameters out of
 * range, are SOCCER_E_INVALID; every call below returns SOCCER_E_STATE during a graph capture.  A learner's memory
 * belongs to its handle: soccer_destroy frees the learners that were not destroyed. */
#define SOCCER_MQ_UNIFORM 0
#define SOCCER_MQ_SELF    1
#define SOCCER_MQ_FIXED   2
#define SOCCER_MQ_MAX_LANES (1ull << 22)
typedef struct soccer_minimax_q soccer_minimax_q;
typedef struct soccer_minimax_q_config {
    double  discount_factor;        /* [0, 1) */
    double  alpha;                  /* initial learning rate, [0, 1] (Littman: 1.0) */
    double  decay;                  /* alpha's factor per learner step, (0, 1] (Littman: 0.01 ** (1 / 1e6)) */
    double  explor;                 /* [0, 1] probability mass spread uniformly over the five actions (Littman: 0.2) */
    double  q_init;                 /* [-1, 1] (Littman: 1.0) */
    int32_t opponent;               /* SOCCER_MQ_* : how player B acts */
    int32_t reserved_;              /* 0 */
    const double* opponent_policy;  /* SOCCER_MQ_FIXED: HOST [n_states][5] rows >= 0 summing to 1; else NULL */
} soccer_minimax_q_config;
int soccer_minimax_q_create(soccer_handle* h, const soccer_minimax_q_config* cfg, soccer_minimax_q** out);
int soccer_minimax_q_destroy(soccer_handle* h, soccer_minimax_q* q);
/* n_steps learner steps, two launches each, enqueued on the handle's stream: no synchronisation, no copy.  Consumes n_steps ticks. */
int soccer_minimax_q_run(soccer_handle* h, soccer_minimax_q* q, int32_t n_steps);
/* steps 3-6 on the caller's batch of n <= 2^22 transitions (DEVICE pointers, n elements each; n = 0: steps 4-6 alone).
 * A transition with an action byte outside 0..4 (SOCCER_MISUSE_ACTION) or with obs = 0, obs >= n_states or
 * next_obs >= n_states (SOCCER_MISUSE_OBSERVATION) sets the sticky flag and is left out.  Consumes no tick. */
int soccer_minimax_q_update(soccer_handle* h, soccer_minimax_q* q, int64_t n, const uint16_t* obs, const int8_t* act_a,
                            const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs);
/* HOST outputs, any may be NULL: Q[n_states][5][5], V[n_states], pi_a / pi_b [n_states][5], visits[n_states][25].  Synchronises. */
int soccer_minimax_q_read(soccer_handle* h, soccer_minimax_q* q, double* Q, double* V, double* pi_a, double* pi_b,
                          uint64_t* visits, double* alpha, uint64_t* steps);
/* Resume from a checkpoint: HOST Q[n_states][5][5] in (row 0 is taken as zeros), V and the strategies re-solved on the
 * device.  visits (HOST [n_states][25], or NULL: every state counts as visited and the table is left as it is) restores
 * the counts, and a state without a visit gets what creation gives it — V = Q[s][0][0], uniform strategies — not the
 * solver's answer, so that read -> load on a fresh learner continues bit for bit.  alpha / steps: HOST, NULL = unchanged. */
int soccer_minimax_q_load(soccer_handle* h, soccer_minimax_q* q, const double* Q, const uint64_t* visits,
                          const double* alpha, const uint64_t* steps);
/* ---- learners, independent Q (two-player handles; ordinary Q-learning for BOTH players, Littman 1994's baseline and challenger)
 * Lives where a minimax-Q learner lives: a two-player SOCCER_F_AUTORESET handle of at most 2^22 lanes, whose lanes are its
 * actors.  It keeps TWO float64 tables on the device, Q_a[n_states][5] over player A's actions in player A's reward and
 * Q_b[n_states][5] over player B's in player B's OWN reward (-r, as the reference's learner-B table is), visits[n_states][25]
 * (uint64, joint cell s * 25 + a * 5 + b), alpha and a step counter.  Derived, never state of their own:
 *     V_p[s] = max_k Q_p[s][k],  g_p[s] = the first k that attains it,  Vq_p[s] = rint(V_p[s] * 2^40) as int64
 * Row 0 is the terminal observation: Q_p[0] = 0 for good.
 * How a player acts (soccer_q_learner_config::act_a / act_b):
 *   SOCCER_QL_GREEDY   epsilon-greedy on its own table: the threshold row of (1.0 - explor) * onehot(g_p[s]) + explor / 5.0,
 *                      by the expression of step 1 above
 *   SOCCER_QL_UNIFORM  the NULL row table of batched_rollout, i.e. its (h * 5) >> 15 draw (NOT the thresholds of a 0.2 row,
 *                      which differ at h = 6553)
 *   SOCCER_QL_FIXED    the thresholds of the caller's mixed policy (policy_a / policy_b), computed once at creation
 * Q-learning is off-policy: BOTH tables are always updated, however the players act.  So (GREEDY, UNIFORM) is Littman's QR,
 * (GREEDY, GREEDY) his QQ, (FIXED, GREEDY) a challenger against a frozen pi_a (read Q_b) and (GREEDY, FIXED) one against a
 * frozen pi_b (read Q_a).  One learner step, in this order:
 *   1. the behaviour rows as above
 *   2. act and step: batched_rollout(n_steps = 1, sample_actions = 1, mix_a, mix_b), exactly as step 2 of minimax-Q
 *   3. reduce, INTEGER sums only:  for A, per (s, a):  c = samples, R = sum of r, SV = sum over the non-terminated samples of
 *      Vq_a[s'];  for B, per (s, b):  c, R = sum of (-r), SV = sum of Vq_b[s']
 *   4. update, for every (s, k) with c > 0:  m = ((double)R + discount_factor * ((double)SV * 2^-40)) / (double)c,
 *      Q = Q + alpha * (m - Q), not contracted;  visits[joint cell] += that cell's count
 *   5. V_p, Vq_p, g_p and the GREEDY players' threshold rows follow Q for the touched states
 *   6. alpha = alpha * decay, steps += 1
 * Initially Q_p[s] = q_init on the live states, so every greedy action is 0 by the first-index rule; nothing is "set, not
 * solved": the learner's whole state is (Q_a, Q_b, visits, alpha, steps), a fixed function of (seed, parameters, number of
 * steps).  With alpha and q_init in range and discount_factor < 1 every Q stays in [-1, 1], and the sums of 2^22 samples fit
 * int64 as they do for minimax-Q.  Ranges, refusals, SOCCER_E_STATE during a capture, the misuse flags and the ownership of
 * the memory are those of the soccer_minimax_q_* calls; both kinds of learner may live on one handle. */
#define SOCCER_QL_GREEDY  0
#define SOCCER_QL_UNIFORM 1
#define SOCCER_QL_FIXED   2
typedef struct soccer_q_learner soccer_q_learner;
typedef struct soccer_q_learner_config {
    double  discount_factor;        /* [0, 1) */
    double  alpha;                  /* initial learning rate, [0, 1] */
    double  decay;                  /* alpha's factor per learner step, (0, 1] */
    double  explor;                 /* [0, 1] probability mass a GREEDY player spreads uniformly over the five actions */
    double  q_init;                 /* [-1, 1] */
    int32_t act_a;                  /* SOCCER_QL_* : how player A acts */
    int32_t act_b;                  /* SOCCER_QL_* : how player B acts */
    const double* policy_a;         /* act_a == SOCCER_QL_FIXED: HOST [n_states][5] rows >= 0 summing to 1; else NULL */
    const double* policy_b;         /* the same for act_b */
} soccer_q_learner_config;
int soccer_q_learner_create(soccer_handle* h, const soccer_q_learner_config* cfg, soccer_q_learner** out);
int soccer_q_learner_destroy(soccer_handle* h, soccer_q_learner* q);
/* n_steps learner steps, two launches each, enqueued on the handle's stream: no synchronisation, no copy.  Consumes n_steps ticks. */
int soccer_q_learner_run(soccer_handle* h, soccer_q_learner* q, int32_t n_steps);
/* steps 3-6 on the caller's batch of n <= 2^22 transitions (DEVICE pointers; reward is player A's), with the checks and the
 * misuse flags of soccer_minimax_q_update.  Consumes no tick. */
int soccer_q_learner_update(soccer_handle* h, soccer_q_learner* q, int64_t n, const uint16_t* obs, const int8_t* act_a,
                            const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs);
/* HOST outputs, any may be NULL: Q_a / Q_b [n_states][5], visits[n_states][25].  Synchronises. */
int soccer_q_learner_read(soccer_handle* h, soccer_q_learner* q, double* Q_a, double* Q_b, uint64_t* visits,
                          double* alpha, uint64_t* steps);
/* Resume from a checkpoint: HOST Q_a / Q_b [n_states][5] in [-1, 1] (row 0 is taken as zeros); every derived row is
 * recomputed from them.  visits: HOST [n_states][25], or NULL: the counts are zeroed.  alpha / steps: HOST, NULL = unchanged. */
int soccer_q_learner_load(soccer_handle* h, soccer_q_learner* q, const double* Q_a, const double* Q_b, const uint64_t* visits,
                          const double* alpha, const uint64_t* steps);
/* ---- learners, policy hill-climbing (two-player handles; PHC and WoLF-PHC, "win or learn fast", Bowling & Veloso 2002)
 * Lives where the other two learners live: a two-player SOCCER_F_AUTORESET handle of at most 2^22 lanes, whose lanes are its
 * actors.  Besides the Q-learners' two tables it keeps an explicit MIXED policy per player and moves it a small step towards
 * the greedy action after every update: a small step while the policy does better than its own average, a large one while
 * it does worse.  State, float64 unless noted:
 *     Q_a[n_states][5], Q_b[n_states][5] (Q_b in player B's own reward), pi_a, pi_b, avg_a, avg_b [n_states][5] (the policies
 *     and their running averages), visits[n_states][25] (uint64), updates[n_states] (uint64: the learner steps in which the
 *     state was touched), alpha, dscale (the factor on both deltas), steps
 * Derived, never state of their own: V_p, g_p, Vq_p as for the Q-learners, and the threshold rows.
 * Row 0 is the terminal observation: Q_p[0] = 0 for good; row 0 of pi and avg is 0.2 at creation (a FIXED player's is the
 * caller's) and is never read or written again.
 * How a player acts (soccer_wolf_phc_config::act_a / act_b):
 *   SOCCER_PHC_LEARN    it draws from the threshold row of (1.0 - explor) * pi_p[s][k] + explor / 5.0 (step 1 of minimax-Q);
 *                       its pi and avg are updated
 *   SOCCER_PHC_UNIFORM  the NULL row table, as SOCCER_QL_UNIFORM; pi_p = avg_p = 0.2 rows, constant
 *   SOCCER_PHC_FIXED    the thresholds of the caller's mixed policy, computed once and checked like opponent_policy;
 *                       pi_p = avg_p = that policy, constant
 * One learner step, in this order:
 *   1. the behaviour rows as above
 *   2. act and step: batched_rollout(n_steps = 1, sample_actions = 1, mix_a, mix_b), exactly as step 2 of the Q-learners
 *   3. reduce: the Q-learners' step 3
 *   4. Q update: the Q-learners' step 4, for both tables whatever the modes; visits grow by the cell counts
 *   5. policy step, for every live state s with any touched joint cell:  updates[s] += 1 (once per state, whatever the
 *      modes), n = (double)updates[s];  then for each LEARN player, with Q = Q_p[s] AFTER step 4, every operation sequential
 *      float64 and not contracted:
 *        avg[k] = avg[k] + (pi[k] - avg[k]) / n                          for k = 0..4
 *        ep = sum_k pi[k] * Q[k],  ea = sum_k avg[k] * Q[k]              each as acc = acc + p * q from 0.0 in index order,
 *                                                                        ea with the NEW avg
 *        d = ((ep > ea ? delta_win : delta_lose) * dscale) / 4.0
 *        g = the first k attaining max_k Q[k]
 *        moved = 0.0;  for k = 0..4, k != g, in index order:  m = min(pi[k], d),  pi[k] = pi[k] - m,  moved = moved + m
 *        pi[g] = pi[g] + moved
 *      Vq_p[s] and a LEARN player's threshold row follow
 *   6. alpha = alpha * decay, dscale = dscale * delta_decay, steps += 1
 * Initially Q_p = q_init on the live states, pi = avg = 0.2, updates = visits = 0, dscale = 1.0.  delta_win == delta_lose
 * is plain PHC.  Rows of pi stay >= 0 exactly (pi[k] - min(pi[k], d) >= 0) and sum to 1 up to rounding, far inside the 1e-5
 * that soccer_best_response's row check allows, and avg is a convex combination of such rows: what soccer_wolf_phc_read
 * returns goes straight into soccer_best_response and into soccer_rollout_args::mix_*.  The learner's state is a fixed
 * function of (seed, parameters, number of steps).  Ranges, refusals, SOCCER_E_STATE during a capture, the misuse flags and
 * the ownership of the memory are those of the soccer_q_learner_* calls; all three kinds of learner may live on one handle. */
#define SOCCER_PHC_LEARN   0
#define SOCCER_PHC_UNIFORM 1
#define SOCCER_PHC_FIXED   2
typedef struct soccer_wolf_phc soccer_wolf_phc;
typedef struct soccer_wolf_phc_config {
    double  discount_factor;        /* [0, 1) */
    double  alpha;                  /* initial learning rate, [0, 1] */
    double  decay;                  /* alpha's factor per learner step, (0, 1] */
    double  explor;                 /* [0, 1] probability mass a LEARN player spreads uniformly over the five actions */
    double  q_init;                 /* [-1, 1] */
    double  delta_win;              /* [0, 1] policy step while ep > ea (Bowling & Veloso: delta_lose / 4 or so) */
    double  delta_lose;             /* [0, 1] policy step otherwise */
    double  delta_decay;            /* dscale's factor per learner step, (0, 1] */
    int32_t act_a;                  /* SOCCER_PHC_* : how player A acts */
    int32_t act_b;                  /* SOCCER_PHC_* : how player B acts */
    const double* policy_a;         /* act_a == SOCCER_PHC_FIXED: HOST [n_states][5] rows >= 0 summing to 1; else NULL */
    const double* policy_b;         /* the same for act_b */
} soccer_wolf_phc_config;
/* what soccer_wolf_phc_read fills and soccer_wolf_phc_load takes: HOST pointers, any may be NULL */
typedef struct soccer_wolf_phc_state {
    double* Q_a; double* Q_b;       /* [n_states][5] */
    double* pi_a; double* pi_b;     /* [n_states][5] */
    double* avg_a; double* avg_b;   /* [n_states][5] */
    uint64_t* visits;               /* [n_states][25] */
    uint64_t* updates;              /* [n_states] */
    double* alpha; double* dscale;  /* one value each */
    uint64_t* steps;
} soccer_wolf_phc_state;
int soccer_wolf_phc_create(soccer_handle* h, const soccer_wolf_phc_config* cfg, soccer_wolf_phc** out);
int soccer_wolf_phc_destroy(soccer_handle* h, soccer_wolf_phc* q);
/* n_steps learner steps, two launches each, enqueued on the handle's stream: no synchronisation, no copy.  Consumes n_steps ticks. */
int soccer_wolf_phc_run(soccer_handle* h, soccer_wolf_phc* q, int32_t n_steps);
/* steps 3-6 on the caller's batch of n <= 2^22 transitions (DEVICE pointers; reward is player A's), with the checks and the
 * misuse flags of soccer_minimax_q_update.  Consumes no tick. */
int soccer_wolf_phc_update(soccer_handle* h, soccer_wolf_phc* q, int64_t n, const uint16_t* obs, const int8_t* act_a,
                           const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs);
/* Fills every array `out` points to.  Synchronises. */
int soccer_wolf_phc_read(soccer_handle* h, soccer_wolf_phc* q, const soccer_wolf_phc_state* out);
/* Resume from a checkpoint; nothing of `in` is written.  Q_a / Q_b are required, in [-1, 1], row 0 taken as zeros.  pi_p /
 * avg_p of a LEARN player: rows 1.. must be >= 0 and sum to 1 as a fixed policy's must (SOCCER_E_INVALID, the message names
 * array and state), row 0 is not read, NULL = left as it is; those of a player that does not LEARN are ignored.  visits /
 * updates: NULL = the counts are zeroed.  alpha, dscale (both in [0, 1]) and steps: NULL = unchanged.  Every derived row is
 * recomputed, so read -> load on a fresh learner continues bit for bit. */
int soccer_wolf_phc_load(soccer_handle* h, soccer_wolf_phc* q, const soccer_wolf_phc_state* in);
/* ---- learners, a population of independent Q-learners (two-player handles; a learner per lane)
 * The three learners above keep ONE table per handle and every lane feeds it.  A population keeps n tables: on a two-player
 * SOCCER_F_AUTORESET handle of n lanes it has n members, and member i is exactly a soccer_q_learner whose only actor is lane
 * i of the handle — the protocol of one learner, one stream of experience, many independent runs (seeds come from the lanes'
 * own Philox streams, hyperparameters may differ per member).  Member i has its own float64 Q_a[n_states][5] and
 * Q_b[n_states][5] (Q_b in player B's own reward, row 0 zero for good) and its own alpha; the population has one step counter.
 * No visits are kept (at [n_states][25] uint64 they would be 2.5 times the tables).
 * One step of member i is steps 1-6 of "learners, independent Q" on the single transition of lane i:
 *   1. the behaviour rows from ITS tables at the lane's observation: SOCCER_QL_GREEDY (with its own explor), SOCCER_QL_UNIFORM
 *      or SOCCER_QL_FIXED, with the same meanings and the same threshold expression; a FIXED player's policy is one
 *      [n_states][5] array shared by all members
 *   2. act and step: batched_rollout(n_steps = 1, sample_actions = 1) with that lane's rows
 *   3.-5. with one sample c = 1, so for (s, a) in Q_a with r and for (s, b) in Q_b with -r:
 *      m = ((double)R + discount_factor * ((double)SV * 2^-40)) / 1.0,  Q = Q + alpha * (m - Q), not contracted, where
 *      SV = terminated ? 0 : Vq_p[s'] and Vq_p[s'] = rint(max_k Q_p[s'][k] * 2^40) is read BEFORE the step's update (it
 *      matters when s' == s); s' = final_obs, so a truncated transition that did not terminate bootstraps from it.  The
 *      2^-40 grid is kept although one sample does not need it: it makes a member bit for bit the learner above
 *   6. alpha_i = alpha_i * decay_i; the step counter grows by one per step of the population
 * A lane that still needs its first reset (SOCCER_MISUSE_FROZEN) and a lane whose current observation is 0 contribute
 * nothing; their member's alpha still advances.  The population's state is a fixed function of (seed, parameters, number of
 * steps): it does not depend on how run() splits its launches or on the state layout.
 * Hyperparameters: the scalars of soccer_q_learner_config for everyone, or — where the pointer is not NULL — HOST arrays of n
 * values, one per member, for alpha, decay, explor and discount_factor (every value in the scalar's range); q_init is scalar.
 * Refusals, SOCCER_E_STATE during a capture, the misuse flags and the ownership of the memory are those of the
 * soccer_q_learner_* calls (no bound on n but memory: n * n_states * 80 bytes of tables, 32 bytes of parameters per member and
 * a shared policy's thresholds; SOCCER_E_NOMEM leaves the handle usable).  Populations and the other learners may share a handle. */
typedef struct soccer_q_population soccer_q_population;
typedef struct soccer_q_population_config {
    double  discount_factor;        /* [0, 1) */
    double  alpha;                  /* initial learning rate, [0, 1] */
    double  decay;                  /* alpha's factor per step, (0, 1] */
    double  explor;                 /* [0, 1] probability mass a GREEDY player spreads uniformly over the five actions */
    double  q_init;                 /* [-1, 1] */
    int32_t act_a;                  /* SOCCER_QL_* : how player A acts */
    int32_t act_b;                  /* SOCCER_QL_* : how player B acts */
    const double* policy_a;         /* act_a == SOCCER_QL_FIXED: HOST [n_states][5] rows >= 0 summing to 1; else NULL */
    const double* policy_b;         /* the same for act_b */
    const double* alpha_per_member;            /* HOST [n_lanes] or NULL: `alpha` for everyone */
    const double* decay_per_member;            /* HOST [n_lanes] or NULL */
    const double* explor_per_member;           /* HOST [n_lanes] or NULL */
    const double* discount_factor_per_member;  /* HOST [n_lanes] or NULL */
} soccer_q_population_config;
int soccer_q_population_create(soccer_handle* h, const soccer_q_population_config* cfg, soccer_q_population** out);
int soccer_q_population_destroy(soccer_handle* h, soccer_q_population* q);
/* n_steps steps of every member in ceil(n_steps / K) launches of at most K steps each (K = 4096, the rollout's own bound; the
 * environment variable SOCCER_POP_LAUNCH_STEPS, read at creation, overrides it: tests of the launch boundary), enqueued on the
 * handle's stream: no synchronisation, no copy.  Consumes n_steps ticks.  A second test hook: SOCCER_POP_GRID_BLOCKS, read at
 * creation and accepted in 1..the handle's grid cap, caps the workgroups of this population's run and update launches (tests
 * of a thread that serves several members in turn); it changes no result. */
int soccer_q_population_run(soccer_handle* h, soccer_q_population* q, int32_t n_steps);
/* steps 3-6 on the caller's transitions: DEVICE arrays of n_lanes elements, transition i belongs to member i (reward is
 * player A's), with the checks and the misuse flags of soccer_q_learner_update: a bad transition leaves its member's tables
 * alone (its alpha still advances).  Consumes no tick. */
int soccer_q_population_update(soccer_handle* h, soccer_q_population* q, const uint16_t* obs, const int8_t* act_a,
                               const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs);
/* Members first .. first + count - 1 (inside the population, else SOCCER_E_INVALID) to HOST arrays, any may be NULL:
 * Q_a / Q_b [count][n_states][5], alpha[count], steps (one value).  Synchronises. */
int soccer_q_population_read(soccer_handle* h, soccer_q_population* q, int64_t first, int64_t count, double* Q_a, double* Q_b,
                             double* alpha, uint64_t* steps);
/* The same range from HOST arrays, any may be NULL (= unchanged): Q_a / Q_b [count][n_states][5] in [-1, 1] (row 0 is taken
 * as zeros), alpha[count] in [0, 1], steps.  Everything is checked before anything is written: a refused load changes
 * nothing.  read -> load of a range on a fresh population continues bit for bit. */
int soccer_q_population_load(soccer_handle* h, soccer_q_population* q, int64_t first, int64_t count, const double* Q_a,
                             const double* Q_b, const double* alpha, const uint64_t* steps);
/* ---- learners, a league opponent for the population of Q-learners
 * A FIXED player of a population follows ONE policy.  A league player follows a MIXTURE over K policies in the sense of a
 * meta-game (soccer_solve_meta_games): "draw policy j with probability w_j at kick-off and play it to the end of the
 * episode" — not the state-wise average sum_j w_j * pi_j, which is another policy.  It is the opponent of policy-space
 * response oracles (PSRO, double oracle), fictitious self-play and league training.
 * A league is K <= SOCCER_LEAGUE_MAX_POLICIES mixed policies [K][n_states][5], one weight vector w[K] shared by all members
 * and the player (0 = A, 1 = B) that plays them.  In the config that player is SOCCER_QL_FIXED with a NULL policy pointer;
 * the other player is anything a population allows.  Member i gains one word of state, pick_i in {-1, 0 .. K - 1}, -1 at
 * creation.  One step of member i at tick t is steps 1-6 of the population with one addition before step 1 and one after
 * the environment step:
 *   0. if pick_i == -1 (whether or not the lane is frozen or parked at observation 0), a pick is drawn from W, the lane's
 *      word of block(2^62 + t, 1) (global lane g = lane_offset + i, word g & 3):
 *          pick_i = #{k < K - 1 : W >= T_k},   T_k = min(2^32, floor(c_k * 2^32)) as an integer,
 *          c_k = w_0 + .. + w_k, summed sequentially in float64
 *      (how the count is found is no part of the definition: the kernel bisects the never decreasing T)
 *   1. the league player's row is the threshold row of policies[pick_i][s], computed on the host at creation by the fixed
 *      policies' own threshold expression; the other player's row as before
 *   2.-6. as before; and after the environment step, if the lane's episode finished (terminated or truncated: the
 *      auto-reset happened), pick_i = -1
 * So a policy of weight zero is never picked (T_k = T_{k-1}); with a trailing zero weight the last policy is unreachable
 * whenever c_{K-2} >= 1; the pick survives launch boundaries; soccer_q_population_update never touches it; a frozen lane
 * draws once, at its first run step, and keeps that pick.  A batched_reset by the CALLER does not redraw it either: the
 * lane's new episode goes on with the pick of the one the caller cut short (load -1 to redraw).
 * Checks, SOCCER_E_INVALID with the reason: the weights as a policy row is — finite, >= 0 (the message names the index),
 * |sum - 1| <= 1e-8 + 1e-5; every policy as policy_a / policy_b are (the message names policy and state); K < 1,
 * K > SOCCER_LEAGUE_MAX_POLICIES; a league player that is not FIXED-with-NULL.  Every other soccer_q_population_* call
 * works on a league population unchanged (run, update, read, load, destroy, SOCCER_POP_LAUNCH_STEPS,
 * SOCCER_POP_GRID_BLOCKS); the league calls on a population without one return SOCCER_E_INVALID.  Memory: K * n_states * 8
 * bytes of thresholds, 8 * (K - 1) bytes of T and 4 bytes per member.  Not offered: per-member weights, new weights for
 * a live population, leagues in the other two populations, per-(member, policy) tallies. */
#define SOCCER_LEAGUE_MAX_POLICIES 1024
int soccer_q_population_create_league(soccer_handle* h, const soccer_q_population_config* cfg, int32_t league_player,
                                      int32_t n_policies, const double* policies /* HOST [K][n_states][5] */,
                                      const double* weights /* HOST [K] */, soccer_q_population** out);
/* Members first .. first + count - 1 to HOST pick[count].  Synchronises. */
int soccer_q_population_league_read(soccer_handle* h, soccer_q_population* q, int64_t first, int64_t count, int32_t* pick);
/* The same range from HOST pick[count], every value in -1 .. K - 1, checked before anything is written: a refused load
 * changes nothing.  read + league_read -> load + league_load on a fresh population continues bit for bit, mid-episode
 * included. */
int soccer_q_population_league_load(soccer_handle* h, soccer_q_population* q, int64_t first, int64_t count, const int32_t* pick);

/* ---- learners, a population of policy hill-climbers (two-player handles; a PHC / WoLF-PHC learner per lane)
 * What the population of Q-learners is to soccer_q_learner, this is to soccer_wolf_phc; nothing new is defined.  On a
 * two-player SOCCER_F_AUTORESET handle of n lanes the population has n members, and member i is exactly a soccer_wolf_phc
 * learner whose only actor is lane i, bit for bit: Bowling & Veloso's protocol of one learner, one stream, many trials.
 * State of member i, float64 unless noted: Q_a, Q_b, pi_a, pi_b, avg_a, avg_b [n_states][5], updates[n_states] (uint64),
 * alpha_i, dscale_i.  The population has one step counter.  No visits are kept, as in the population of Q-learners.
 * Row 0 as for soccer_wolf_phc: Q_p[0] = 0 for good, row 0 of pi and avg is never read by a step.
 * One step of member i is steps 1-6 of "learners, policy hill-climbing" on the single transition of lane i:
 *   1. a LEARN player draws from the threshold row of (1.0 - explor_i) * pi_p[s][k] + explor_i / 5.0 of ITS pi at the lane's
 *      observation s; a UNIFORM player from the NULL row table; a FIXED player from the thresholds of its own row pi_p[s]
 *      with explor 0.0 — the same expression, which for explor 0.0 is the host's threshold computation of a fixed policy
 *      operation for operation, so the action is the one the host-computed table of soccer_wolf_phc gives, bit for bit
 *   2. act and step: batched_rollout(n_steps = 1, sample_actions = 1) with that lane's rows
 *   3.-4. the Q update with one sample c = 1 on the 2^-40 grid, exactly as in the population of Q-learners: Vq_p[s'] is read
 *      BEFORE the update, no bootstrap when terminated, s' = final_obs so a truncated transition bootstraps from it
 *   5. updates[s] += 1, n = (double)updates[s]; then the policy step for each LEARN player in the exact operation order of
 *      "learners, policy hill-climbing" with delta_win_i, delta_lose_i and dscale_i.  ep > ea is strict, so the first touch
 *      of a state (pi == avg) is a delta_lose step
 *   6. alpha_i = alpha_i * decay_i, dscale_i = dscale_i * delta_decay_i; the step counter grows by one per step
 * A lane that still needs its first reset (SOCCER_MISUSE_FROZEN) and a lane whose current observation is 0 contribute
 * nothing; their member's alpha and dscale still advance.
 * A FIXED player's policy is PER MEMBER: it lives in that member's pi (= avg) rows, constant under run / update.  Creation
 * takes one shared [n_states][5] policy (policy_p: copied to every member) or a HOST array [n_lanes][n_states][5]
 * (policy_p_per_member), exactly one of the two, checked as opponent_policy is; the message names the member and the state.
 * soccer_wolf_population_adopt writes it on the device from another population.
 * Hyperparameters: the scalars of soccer_wolf_phc_config for everyone, or — where the pointer is not NULL — HOST arrays of n
 * values, one per member, for alpha, decay, explor, discount_factor, delta_win, delta_lose and delta_decay (every value in
 * the scalar's range); q_init is scalar.  The state is a fixed function of (seed, parameters, number of steps): it does not
 * depend on how run() splits its launches or on the state layout.
 * Refusals, SOCCER_E_STATE during a capture, the misuse flags and the ownership of the memory are those of the
 * soccer_q_population_* calls (memory: n * n_states * 256 bytes of rows and 64 bytes of parameters per member;
 * SOCCER_E_NOMEM leaves the handle usable).  Populations of both kinds and the three shared learners may share a handle. */
typedef struct soccer_wolf_population soccer_wolf_population;
typedef struct soccer_wolf_population_config {
    double  discount_factor;        /* the fields of soccer_wolf_phc_config, in place */
    double  alpha;
    double  decay;
    double  explor;
    double  q_init;
    double  delta_win;
    double  delta_lose;
    double  delta_decay;
    int32_t act_a;                  /* SOCCER_PHC_* */
    int32_t act_b;
    const double* policy_a;         /* act_a == SOCCER_PHC_FIXED: HOST [n_states][5], shared by every member; else NULL */
    const double* policy_b;
    const double* policy_a_per_member;         /* or HOST [n_lanes][n_states][5]: a FIXED player has exactly one of the two */
    const double* policy_b_per_member;
    const double* alpha_per_member;            /* HOST [n_lanes] or NULL: `alpha` for everyone */
    const double* decay_per_member;
    const double* explor_per_member;
    const double* discount_factor_per_member;
    const double* delta_win_per_member;
    const double* delta_lose_per_member;
    const double* delta_decay_per_member;
} soccer_wolf_population_config;
/* what soccer_wolf_population_read fills and soccer_wolf_population_load takes for `count` members: HOST pointers, any may
 * be NULL; soccer_wolf_phc_state with a leading dimension and without visits */
typedef struct soccer_wolf_population_state {
    double* Q_a; double* Q_b;       /* [count][n_states][5] */
    double* pi_a; double* pi_b;     /* [count][n_states][5] */
    double* avg_a; double* avg_b;   /* [count][n_states][5] */
    uint64_t* updates;              /* [count][n_states] */
    double* alpha; double* dscale;  /* [count] */
    uint64_t* steps;                /* one value */
} soccer_wolf_population_state;
int soccer_wolf_population_create(soccer_handle* h, const soccer_wolf_population_config* cfg, soccer_wolf_population** out);
int soccer_wolf_population_destroy(soccer_handle* h, soccer_wolf_population* q);
/* n_steps steps of every member in ceil(n_steps / K) launches (K = 4096; SOCCER_POP_LAUNCH_STEPS, read at creation, overrides
 * it as for soccer_q_population_run), enqueued on the handle's stream: no synchronisation, no copy.  Consumes n_steps ticks.
 * SOCCER_POP_GRID_BLOCKS caps the grid of run and update launches as for soccer_q_population_run. */
int soccer_wolf_population_run(soccer_handle* h, soccer_wolf_population* q, int32_t n_steps);
/* steps 3-6 on the caller's transitions: DEVICE arrays of n_lanes elements, transition i belongs to member i (reward is
 * player A's).  A bad transition leaves its member's rows alone (its alpha and dscale still advance) and sets the misuse
 * flag.  Consumes no tick. */
int soccer_wolf_population_update(soccer_handle* h, soccer_wolf_population* q, const uint16_t* obs, const int8_t* act_a,
                                  const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs);
/* Members first .. first + count - 1 (inside the population, else SOCCER_E_INVALID) into every array `out` points to.
 * Synchronises. */
int soccer_wolf_population_read(soccer_handle* h, soccer_wolf_population* q, int64_t first, int64_t count,
                                const soccer_wolf_population_state* out);
/* The same range from HOST arrays, any may be NULL (= unchanged): Q_p in [-1, 1] (row 0 is taken as zeros); pi_p / avg_p of a
 * LEARN or FIXED player with rows 1.. >= 0 and summing to 1 as a fixed policy's must (the message names array, member and
 * state; row 0 is not read; those of a UNIFORM player are ignored); updates; alpha and dscale in [0, 1]; steps.  Everything is
 * checked before anything is written: a refused load changes nothing.  read -> load of a range on a fresh population
 * continues bit for bit. */
int soccer_wolf_population_load(soccer_handle* h, soccer_wolf_population* q, int64_t first, int64_t count,
                                const soccer_wolf_population_state* in);
/* The freeze of the challenger protocol: copies, member by member, on the device and in stream order, src's pi (which = 0) or
 * avg (which = 1) of src_player (0 = A, 1 = B) into dst's pi AND avg of dst_player.  dst_player must be FIXED in dst, src != dst,
 * both populations of this handle, else SOCCER_E_INVALID with the reason.  No host copy, no synchronisation. */
int soccer_wolf_population_adopt(soccer_handle* h, soccer_wolf_population* dst, int32_t dst_player, soccer_wolf_population* src,
                                 int32_t src_player, int32_t which);

/* ---- learners, a population of minimax-Q learners (two-player handles; a minimax-Q learner per lane)
 * What the two populations above are to soccer_q_learner and soccer_wolf_phc, this is to soccer_minimax_q; nothing new is
 * defined.  On a two-player SOCCER_F_AUTORESET handle of n lanes the population has n members, and member i is exactly a
 * soccer_minimax_q learner whose only actor is lane i, bit for bit: Littman's protocol of one learner, one stream of experience,
 * many runs.  State of member i, all float64: Q[n_states][5][5], V[n_states], pi_a / pi_b [n_states][5], alpha_i.  The
 * population has one step counter.  No visits are kept, as in the other populations.
 * Row 0 is the terminal observation: Q[0] = V[0] = 0 for good.  Creation gives Q = V = q_init on the live states and uniform
 * strategies, SET, NOT SOLVED: a state's strategies are first solved when the state is first updated, so pi_a and pi_b are
 * state kept in memory and cannot be recomputed from Q.
 * One step of member i is steps 1-6 of "learners (minimax-Q)" on the single transition of lane i:
 *   1. player A draws from the threshold row of (1.0 - explor_i) * pi_a[s][k] + explor_i / 5.0 of ITS pi_a at the lane's
 *      observation s (the expression of step 1 there); player B by `opponent`: SOCCER_MQ_UNIFORM the NULL row table,
 *      (h * 5) >> 15; SOCCER_MQ_SELF the same expression on its pi_b[s]; SOCCER_MQ_FIXED the host-computed thresholds of a
 *      fixed mixed policy, one [n_states][5] array shared by all members (opponent_policy) or one per member
 *      (opponent_policy_per_member, [n_lanes][n_states][5]): exactly one of the two, checked as opponent_policy of
 *      soccer_minimax_q_config is; the message names the member and the state
 *   2. act and step: batched_rollout(n_steps = 1, sample_actions = 1) with that lane's rows — the same tick and Philox
 *      words, auto-reset, episode histogram and misuse flags as for the other populations
 *   3.-4. with one sample c = 1, on the cell (s, a, b):  m = (double)r + discount_factor_i * ((double)SV * 2^-40) where
 *      SV = terminated ? 0 : rint(V[s'] * 2^40),  Q = Q + alpha_i * (m - Q), not contracted.  V[s'] is read BEFORE the step's
 *      re-solve (it matters when s' == s); s' = final_obs, so a truncated transition that did not terminate bootstraps from
 *      it.  The 2^-40 grid is kept so that a member is bit for bit the shared learner with one lane
 *   5. re-solve: (V[s], pi_a[s], pi_b[s]) = solve(Q[s]) (csrc/soccer_games.hpp), that one state, on every learning step
 *   6. alpha_i = alpha_i * decay_i; the step counter grows by one per step of the population
 * A lane that still needs its first reset (SOCCER_MISUSE_FROZEN) and a lane whose current observation is 0 contribute
 * nothing; their member's alpha still advances.  The population's state is a fixed function of (seed, parameters, number of
 * steps): it does not depend on how run() splits its launches, on the launch geometry or on the state layout.
 * Hyperparameters: the scalars of soccer_minimax_q_config for everyone, or — where the pointer is not NULL — HOST arrays of n
 * values, one per member, for alpha, decay, explor and discount_factor (every value in the scalar's range); q_init is scalar.
 * Refusals, SOCCER_E_STATE during a capture, the misuse flags and the ownership of the memory are those of the
 * soccer_q_population_* calls (memory: n * n_states * 288 bytes of rows, 32 bytes of parameters per member and 8 * n_states
 * bytes of thresholds per fixed policy; SOCCER_E_NOMEM leaves the handle usable).  Populations of all three kinds and the
 * three shared learners may share a handle. */
typedef struct soccer_minimax_q_population soccer_minimax_q_population;
typedef struct soccer_minimax_q_population_config {
    double  discount_factor;        /* the fields of soccer_minimax_q_config, in place */
    double  alpha;
    double  decay;
    double  explor;
    double  q_init;
    int32_t opponent;               /* SOCCER_MQ_* : how player B acts */
    int32_t reserved_;              /* 0 */
    const double* opponent_policy;             /* SOCCER_MQ_FIXED: HOST [n_states][5], shared by every member; else NULL */
    const double* opponent_policy_per_member;  /* or HOST [n_lanes][n_states][5]: SOCCER_MQ_FIXED has exactly one of the two */
    const double* alpha_per_member;            /* HOST [n_lanes] or NULL: `alpha` for everyone */
    const double* decay_per_member;
    const double* explor_per_member;
    const double* discount_factor_per_member;
} soccer_minimax_q_population_config;
int soccer_minimax_q_population_create(soccer_handle* h, const soccer_minimax_q_population_config* cfg, soccer_minimax_q_population** out);
int soccer_minimax_q_population_destroy(soccer_handle* h, soccer_minimax_q_population* q);
/* n_steps steps of every member in ceil(n_steps / K) launches (K = 4096; SOCCER_POP_LAUNCH_STEPS, read at creation and accepted
 * in 1..4096, overrides it as for soccer_q_population_run), enqueued on the handle's stream: no synchronisation, no copy.
 * Consumes n_steps ticks.  A launch has min(n, W) workgroups of one wave, a wave per member; beyond W members (W = the waves
 * of the other kernels' largest grid, 8 192 on an MI355X) a wave serves several members in turn.  A test hook: the
 * environment variable SOCCER_MQ_POP_WAVES, read at creation and accepted in 1..W, lowers W (tests of a wave that serves
 * several members); it changes no result, and update() and load()'s re-solve use the same bound. */
int soccer_minimax_q_population_run(soccer_handle* h, soccer_minimax_q_population* q, int32_t n_steps);
/* steps 3-6 on the caller's transitions: DEVICE arrays of n_lanes elements, transition i belongs to member i (reward is
 * player A's), with the checks and the misuse flags of soccer_q_population_update: a bad transition leaves its member alone
 * (its alpha still advances).  Consumes no tick. */
int soccer_minimax_q_population_update(soccer_handle* h, soccer_minimax_q_population* q, const uint16_t* obs, const int8_t* act_a,
                                       const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs);
/* Members first .. first + count - 1 (inside the population, else SOCCER_E_INVALID) to HOST arrays, any may be NULL:
 * Q[count][n_states][5][5], V[count][n_states], pi_a / pi_b [count][n_states][5], alpha[count], steps (one value).  Synchronises. */
int soccer_minimax_q_population_read(soccer_handle* h, soccer_minimax_q_population* q, int64_t first, int64_t count, double* Q, double* V,
                                     double* pi_a, double* pi_b, double* alpha, uint64_t* steps);
/* The same range from HOST arrays, any may be NULL (= unchanged): Q and V in [-1, 1] (row 0 is taken as zeros); pi_a / pi_b with
 * rows 1.. >= 0 and summing to 1 as a fixed policy's must (the message names array, member and state; row 0 is not read and
 * stays what creation gave it); alpha[count] in [0, 1]; steps.  Everything is checked before anything is written: a refused
 * load changes nothing.  Q given with NONE of V, pi_a, pi_b: every live state of the range is re-solved on the device from
 * the new Q.  Otherwise whatever is given is stored as it is and nothing is solved — V or a strategy without Q included — so
 * read -> load of a range on a fresh or a running population continues bit for bit, states never updated included. */
int soccer_minimax_q_population_load(soccer_handle* h, soccer_minimax_q_population* q, int64_t first, int64_t count, const double* Q,
                                     const double* V, const double* pi_a, const double* pi_b, const double* alpha, const uint64_t* steps);

/* ---- learners, a population of opponent-modelling Q-learners (two-player handles; a learner per lane)
 * The learner that SEES the other player's action and models it: opponent-modelling Q-learning (Uther & Veloso 1997, on this
 * game), the joint-action learner of Claus & Boutilier (1998); in self-play, fictitious play in a Markov game.  It learns a
 * joint-action table like minimax-Q but solves no stage game: it best-responds to the EMPIRICAL frequencies of the other
 * player's actions in the state.  On a two-player SOCCER_F_AUTORESET handle of n lanes the population has n members, member i
 * fed by lane i alone.  Per member and per player p in {A, B}:
 *     Q_p[n_states][5][5]  float64, index [s][own action][other's action], in p's OWN reward (B's is -r); row 0, the terminal
 *                          observation, is zero for good
 *     C_p[n_states][5]     uint64, how often the OTHER player was seen to take each action at s; row 0 stays zero
 * and the member's alpha; the population has one step counter.  Derived, never state of their own, for (p, s) — one device
 * function computes them for run, update, creation and load:
 *     n   = C[0] + C[1] + C[2] + C[3] + C[4]                                   (uint64)
 *     w_k = n > 0 ? (double)C[k] : 1.0,   N = n > 0 ? (double)n : 5.0          (nothing seen yet: a uniform belief)
 *     W[a] = ((((w_0 * Q[a][0] + w_1 * Q[a][1]) + w_2 * Q[a][2]) + w_3 * Q[a][3]) + w_4 * Q[a][4])
 *            every product and every sum rounded on its own (not contracted), in this order
 *     g   = the first a that attains max_a W[a]
 *     V   = min(1.0, max(-1.0, W[g] / N))
 *     Vq  = rint(V * 2^40) as int64, the learners' grid
 * The clamp is what makes "Q stays in [-1, 1]" provable whatever the counts: while n < 2^53 rounding is monotone and
 * |W[g]| <= N, but counts beyond that (a load takes them as given) round one by one, and the rounded weights may sum to more
 * than the rounded n — C = (2^53 + 3, 2, 0, 0, 0) with a row of ones gives W[g] / N > 1; with |V| <= 1 a target m = r + discount_factor * V has |m| <= 1 (r is not 0 only where the transition
 * terminated and nothing is bootstrapped), and Q + alpha * (m - Q) stays between Q and m as for the other learners.
 * How a player acts: SOCCER_QL_GREEDY, epsilon-greedy on onehot(g_p[s]) with the member's explor; SOCCER_QL_UNIFORM, the NULL
 * row table, (h * 5) >> 15; SOCCER_QL_FIXED, one [n_states][5] policy shared by all members, its thresholds computed once on
 * the host — the meanings and the threshold expression of "learners, independent Q".  BOTH players' tables and counts are
 * always updated, however they act.  One step of member i on its lane's single transition (s, a, b, r, terminated,
 * s' = final_obs), in the order of "learners, a population of independent Q-learners":
 *   1. the behaviour rows from ITS tables at s
 *   2. act and step: batched_rollout(n_steps = 1, sample_actions = 1) with that lane's rows — the same tick and Philox words,
 *      auto-reset, episode histogram and misuse flags as for the other populations
 *   3. SV_p = terminated ? 0 : Vq_p[s'] for both players, read BEFORE anything moves (it matters when s' == s: every blocked
 *      move, every STAND)
 *   4. for A at cell (a, b):  m = (double)r + discount_factor_i * ((double)SV_A * 2^-40),  Q = Q + alpha_i * (m - Q), not
 *      contracted, then C_A[s][b] += 1;  for B at cell (b, a) the same with -r and SV_B, then C_B[s][a] += 1
 *   5. V, g (and Vq) of (A, s) and (B, s) follow by the function above
 *   6. alpha_i = alpha_i * decay_i; the step counter grows by one per step of the population
 * A lane that still needs its first reset (SOCCER_MISUSE_FROZEN) and a lane whose current observation is 0 contribute
 * nothing; their member's alpha still advances.  Initially Q = q_init on the live states and C = 0, so g = 0 everywhere by
 * the first-index rule.  The population's state is (Q_a, Q_b, C_a, C_b, alpha, steps), a fixed function of (seed,
 * parameters, number of steps): it does not depend on how run() splits its launches, on the grid or on the state layout.
 * Hyperparameters: those of soccer_q_population_config, with the same ranges and the same per-member HOST arrays.
 * Refusals, SOCCER_E_STATE during a capture, the misuse flags and the ownership of the memory are those of the
 * soccer_q_population_* calls (memory: n * n_states * 512 bytes of rows — 390 KB per member on 5x4 —, 32 bytes of parameters
 * per member and a shared policy's thresholds; SOCCER_E_NOMEM leaves the handle usable).  Populations of all kinds and the
 * three shared learners may share a handle.  Not offered: a league opponent, decayed or windowed counts, a shared-table
 * form. */
typedef struct soccer_om_population soccer_om_population;
typedef struct soccer_om_population_config {
    double  discount_factor;        /* the fields of soccer_q_population_config, in place */
    double  alpha;
    double  decay;
    double  explor;
    double  q_init;
    int32_t act_a;                  /* SOCCER_QL_* : how player A acts */
    int32_t act_b;                  /* SOCCER_QL_* : how player B acts */
    const double* policy_a;         /* act_a == SOCCER_QL_FIXED: HOST [n_states][5] rows >= 0 summing to 1; else NULL */
    const double* policy_b;         /* the same for act_b */
    const double* alpha_per_member;            /* HOST [n_lanes] or NULL: `alpha` for everyone */
    const double* decay_per_member;
    const double* explor_per_member;
    const double* discount_factor_per_member;
} soccer_om_population_config;
int soccer_om_population_create(soccer_handle* h, const soccer_om_population_config* cfg, soccer_om_population** out);
int soccer_om_population_destroy(soccer_handle* h, soccer_om_population* q);
/* n_steps steps of every member in ceil(n_steps / K) launches of at most K = 4096 steps each, enqueued on the handle's stream:
 * no synchronisation, no copy.  Consumes n_steps ticks.  The test hooks SOCCER_POP_LAUNCH_STEPS and SOCCER_POP_GRID_BLOCKS are
 * read at creation as for soccer_q_population_run; they change no result. */
int soccer_om_population_run(soccer_handle* h, soccer_om_population* q, int32_t n_steps);
/* steps 3-6 on the caller's transitions: DEVICE arrays of n_lanes elements, transition i belongs to member i (reward is
 * player A's), with the checks and the misuse flags of soccer_q_population_update: a bad transition leaves its member's
 * tables and counts alone (its alpha still advances).  Consumes no tick. */
int soccer_om_population_update(soccer_handle* h, soccer_om_population* q, const uint16_t* obs, const int8_t* act_a,
                                const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs);
/* Members first .. first + count - 1 (inside the population, else SOCCER_E_INVALID) to HOST arrays, any may be NULL:
 * Q_a / Q_b [count][n_states][5][5], C_a / C_b [count][n_states][5] uint64, alpha[count], steps (one value).  Synchronises. */
int soccer_om_population_read(soccer_handle* h, soccer_om_population* q, int64_t first, int64_t count, double* Q_a, double* Q_b,
                              uint64_t* C_a, uint64_t* C_b, double* alpha, uint64_t* steps);
/* The same range from HOST arrays, any may be NULL (= unchanged): Q_a / Q_b in [-1, 1], C_a / C_b taken as given (row 0
 * of all four is taken as zeros), alpha[count] in [0, 1], steps.  Everything is checked before anything is written: a refused load changes
 * nothing.  Every derived value of the range is recomputed on the device by the function above, so read -> load of a range
 * on a fresh population continues bit for bit. */
int soccer_om_population_load(soccer_handle* h, soccer_om_population* q, int64_t first, int64_t count, const double* Q_a,
                              const double* Q_b, const uint64_t* C_a, const uint64_t* C_b, const double* alpha, const uint64_t* steps);

/* ---- learners, a population of regret matchers (two-player handles; a regret-matching learner per lane)
 * Regret matching (Hart & Mas-Colell 2000) per state, the "local no-regret" learner of Kash, Sullins & Hofmann (2020), the
 * dynamic behind CFR and CFR+: Q-values stand in for counterfactual values, the policy is the normalised positive part of the
 * cumulative regrets, and the AVERAGE policy is the one that carries the guarantee.  On a two-player SOCCER_F_AUTORESET handle
 * of n lanes the population has n members, member i fed by lane i alone.  State of member i, float64 unless noted, per player
 * p in {A, B}: Q_p[n_states][5] (B's in its own reward, -r), the cumulative regrets R_p[n_states][5], the policy sums
 * Z_p[n_states][5]; updates[n_states] (uint64); alpha_i.  The population has one step counter.  Creation gives Q = q_init on the
 * live states and 0 in row 0, R = Z = 0, updates = 0.  Two flags hold for the whole population: `plus` (regret matching+: the
 * regrets are floored at 0) and `linear` (a step's policy is weighed by the state's visit count, CFR+'s averaging).
 * A player is SOCCER_PHC_LEARN, SOCCER_PHC_UNIFORM or SOCCER_PHC_FIXED (the hill-climbers' constants, with their meanings); a
 * FIXED player's policy is one [n_states][5] array shared by all members (policy_p) or a HOST array [n_lanes][n_states][5]
 * (policy_p_per_member), exactly one of the two, checked as a fixed policy is; it is constant for the population's life.  BOTH
 * Q tables always learn, however the players act.
 * All arithmetic is float64, one operation at a time, never contracted.
 *   policy(p, s), the row a player acts from before exploration:
 *     LEARN:    pos[k] = R_p[s][k] > 0.0 ? R_p[s][k] : 0.0
 *               tot    = (((((0.0 + pos[0]) + pos[1]) + pos[2]) + pos[3]) + pos[4])
 *               pi[k]  = tot > 0.0 ? pos[k] / tot : 0.2
 *     UNIFORM:  0.2 everywhere
 *     FIXED:    the caller's row at s
 * One step of member i on its lane's transition (s, a, b, r, terminated, s' = final_obs):
 *   0. draw and step as the other populations do, the same Philox words and 15-bit halves: a LEARN player from the threshold
 *      row of (1.0 - explor_i) * pi[k] + explor_i / 5.0 with pi = policy(p, s); a FIXED player the same with explor 0.0; a
 *      UNIFORM player from the NULL row table, (h * 5) >> 15; batched_rollout(n_steps = 1, sample_actions = 1) with those rows
 *   1. pi_p = policy(p, s) and pi'_p = policy(p, s') for both players; every read of row s' happens before any store of this
 *      step (s' may be s)
 *   2. for both players:  v = terminated ? 0.0 : sum_k pi'_p[k] * Q_p[s'][k], accumulated from 0.0 in k order;
 *      m = (double)r_p + discount_factor_i * v with r_A = r, r_B = -r;  Q_p[s][act_p] = old + alpha_i * (m - old).  The
 *      bootstrap is the value of the player's own current policy: not the maximum, and not quantised.  A truncated
 *      transition that did not terminate bootstraps like any other
 *   3. updates[s] += 1, n = (double)updates[s]
 *   4. for each LEARN player, with the row of Q just written:  u = sum_k pi_p[k] * Q_p[s][k], accumulated from 0.0 in k
 *      order;  for every k:  R_p[s][k] = R_p[s][k] + (Q_p[s][k] - u);  under `plus`  R = R > 0.0 ? R : 0.0;
 *      Z_p[s][k] = Z_p[s][k] + w * pi_p[k] with w = linear ? n : 1.0.  A player that does not learn leaves R and Z untouched
 *   5. alpha_i = alpha_i * decay_i; the step counter grows by one per step of the population
 * A lane that still needs its first reset (SOCCER_MISUSE_FROZEN) and a lane whose current observation is 0 contribute
 * nothing; their member's alpha still advances.  Derived by the reader, never state: pi_p = policy(p, .), and the average
 * policy avg_p[s][k] = Z_p[s][k] / (the sum of Z_p[s], in the order of tot), 0.2 where that sum is 0.  The state is a fixed
 * function of (seed, parameters, number of steps): it does not depend on how run() splits its launches, on the grid or on the
 * state layout.
 * Hyperparameters: scalars for everyone, or — where the pointer is not NULL — HOST arrays of n values, one per member, for
 * alpha, decay, explor and discount_factor (the ranges of soccer_q_population_config); q_init, plus and linear are scalars.
 * Refusals, SOCCER_E_STATE during a capture, the misuse flags and the ownership of the memory are those of the
 * soccer_wolf_population_* calls (memory: n * n_states * 256 bytes of rows, 32 bytes of parameters per member and
 * n_states * 40 bytes per fixed policy; SOCCER_E_NOMEM leaves the handle usable).  Populations of all kinds and the shared
 * learners may share a handle.  Not offered: a league opponent, adopt / challengers, a choice of bootstrap, per-member
 * flags.  (The shared-table form is "learners, regret matching", below.) */
typedef struct soccer_regret_population soccer_regret_population;
typedef struct soccer_regret_population_config {
    double  discount_factor;        /* [0, 1) */
    double  alpha;                  /* initial learning rate, [0, 1] */
    double  decay;                  /* alpha's factor per step, (0, 1] */
    double  explor;                 /* [0, 1] probability mass a LEARN player spreads uniformly over the five actions */
    double  q_init;                 /* [-1, 1] */
    int32_t act_a;                  /* SOCCER_PHC_* */
    int32_t act_b;
    int32_t plus;                   /* 0 or 1: regret matching+ */
    int32_t linear;                 /* 0 or 1: linear averaging */
    const double* policy_a;         /* act_a == SOCCER_PHC_FIXED: HOST [n_states][5], shared by every member; else NULL */
    const double* policy_b;
    const double* policy_a_per_member;         /* or HOST [n_lanes][n_states][5]: a FIXED player has exactly one of the two */
    const double* policy_b_per_member;
    const double* alpha_per_member;            /* HOST [n_lanes] or NULL: `alpha` for everyone */
    const double* decay_per_member;
    const double* explor_per_member;
    const double* discount_factor_per_member;
} soccer_regret_population_config;
/* what soccer_regret_population_read fills and soccer_regret_population_load takes for `count` members: HOST pointers, any
 * may be NULL */
typedef struct soccer_regret_population_state {
    double* Q_a; double* Q_b;       /* [count][n_states][5] */
    double* R_a; double* R_b;       /* [count][n_states][5] */
    double* Z_a; double* Z_b;       /* [count][n_states][5] */
    uint64_t* updates;              /* [count][n_states] */
    double* alpha;                  /* [count] */
    uint64_t* steps;                /* one value */
} soccer_regret_population_state;
int soccer_regret_population_create(soccer_handle* h, const soccer_regret_population_config* cfg, soccer_regret_population** out);
int soccer_regret_population_destroy(soccer_handle* h, soccer_regret_population* q);
/* n_steps steps of every member in ceil(n_steps / K) launches (K = 4096; SOCCER_POP_LAUNCH_STEPS, read at creation, overrides
 * it as for soccer_q_population_run), enqueued on the handle's stream: no synchronisation, no copy.  Consumes n_steps ticks.
 * SOCCER_POP_GRID_BLOCKS caps the grid of run and update launches as for soccer_q_population_run. */
int soccer_regret_population_run(soccer_handle* h, soccer_regret_population* q, int32_t n_steps);
/* steps 1-5 on the caller's transitions: DEVICE arrays of n_lanes elements, transition i belongs to member i (reward is
 * player A's).  A bad transition leaves its member's rows alone (its alpha still advances) and sets the misuse flag.
 * Consumes no tick. */
int soccer_regret_population_update(soccer_handle* h, soccer_regret_population* q, const uint16_t* obs, const int8_t* act_a,
                                    const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs);
/* Members first .. first + count - 1 (inside the population, else SOCCER_E_INVALID) into every array `out` points to (R and Z
 * of a player that does not learn are zeros).  Synchronises. */
int soccer_regret_population_read(soccer_handle* h, soccer_regret_population* q, int64_t first, int64_t count,
                                  const soccer_regret_population_state* out);
/* The same range from HOST arrays, any may be NULL (= unchanged): Q_p in [-1, 1]; R_p finite, and >= 0 under `plus`; Z_p finite
 * and >= 0 (the message names array, member, state and action; R_p and Z_p of a player that does not learn are ignored); row 0
 * of all six is taken as zeros; updates; alpha in [0, 1]; steps.  Everything is checked before anything is written: a refused
 * load changes nothing.  read -> load of a range on a fresh population continues bit for bit. */
int soccer_regret_population_load(soccer_handle* h, soccer_regret_population* q, int64_t first, int64_t count,
                                  const soccer_regret_population_state* in);

/* ---- learners, regret matching (two-player handles; the regret matchers above with ONE table that every lane feeds)
 * What soccer_wolf_phc is to its population, this is to the population of regret matchers: the guarantee of regret matching
 * sits on the AVERAGE policy, and the average needs volume, which a batch gives.  Lives where soccer_wolf_phc lives: a
 * two-player SOCCER_F_AUTORESET handle of at most 2^22 lanes, whose lanes are its actors; it may share the handle with every
 * other learner.  State, float64 unless noted:
 *     Q_a[n_states][5], Q_b[n_states][5] (Q_b in player B's own reward), the cumulative regrets R_a, R_b [n_states][5], the
 *     policy sums Z_a, Z_b [n_states][5], visits[n_states][25] (uint64), updates[n_states] (uint64: the learner steps in which
 *     the state was touched), alpha, steps
 * The flags `plus` (regret matching+: regrets floored at 0) and `linear` (a step's policy weighed by the state's update count)
 * are set at creation.  A player is SOCCER_PHC_LEARN, SOCCER_PHC_UNIFORM or SOCCER_PHC_FIXED, with one HOST [n_states][5] policy
 * for a FIXED player, checked as a fixed policy is.  BOTH Q tables always learn, however the players act.
 * policy(p, s) is that of "learners, a population of regret matchers", word for word: LEARN: the positive part of R_p[s], the
 * sequential sum tot, pos[k] / tot, or 0.2 where tot is not > 0.0; UNIFORM: 0.2; FIXED: the caller's row at s.
 * Derived, never state of their own:
 *     v_p[s] = sum_k policy(p, s)[k] * Q_p[s][k], accumulated from 0.0 in k order;  Vq_p[s] = rint(v_p[s] * 2^40) as int64
 * the value of the player's own current policy on the learners' integer grid; it stands where the Q-learners keep the row
 * maximum.  Row 0 is the terminal observation and never a current state: row 0 of all six tables is 0 for good.
 * One learner step, float64, one operation at a time, never contracted:
 *   1. the behaviour rows: LEARN the threshold row of (1.0 - explor) * policy(p, s)[k] + explor / 5.0 (step 1 of minimax-Q);
 *      FIXED the thresholds of the caller's policy, computed once on the host as soccer_wolf_phc does; UNIFORM the NULL row
 *      table
 *   2. act and step: the Q-learners' step 2 (the same Philox words, 15-bit halves and histogram; lanes that still need their
 *      first reset and lanes whose observation is 0 contribute nothing)
 *   3. reduce: the Q-learners' step 3 into the same four integer accumulators per joint cell, with Vq_p as it stood at the
 *      end of the previous step
 *   4. Q update: the Q-learners' step 4, for both tables; visits grow by the cell counts
 *   5. for every live state s with any touched joint cell:  updates[s] += 1, n = (double)updates[s], w = linear ? n : 1.0;
 *      then for each LEARN player, with pi = policy(p, s) from R AS IT WAS BEFORE this step and Q = Q_p[s] AFTER step 4:
 *        u = sum_k pi[k] * Q[k], accumulated from 0.0 in k order
 *        for every k:  R[k] = R[k] + (Q[k] - u);  under `plus`  R[k] = R[k] > 0.0 ? R[k] : 0.0;  Z[k] = Z[k] + w * pi[k]
 *      (a player that does not learn leaves R and Z untouched: zeros); then, for BOTH players, Vq_p[s] from the new R and
 *      the new Q, and a LEARN player's threshold row
 *   6. alpha = alpha * decay, steps += 1
 * Initially Q_p = q_init on the live states, R = Z = 0 (every LEARN row starts on the 0.2 fallback), the counts 0.  Derived by
 * the reader, never state: pi_p = policy(p, .), and avg_p[s][k] = Z_p[s][k] / (the sum of Z_p[s], in the order of tot), 0.2
 * where that sum is 0.  The state is a fixed function of (seed, parameters, number of steps): it does not depend on the launch
 * split, on the grid or on the state layout.  A one-lane handle is NOT bit for bit a one-member population: the population
 * bootstraps with the unquantised v, this form sums Vq over lanes and must stay on the grid.  Ranges, refusals, SOCCER_E_STATE
 * during a capture, the misuse flags and the ownership of the memory (SOCCER_E_NOMEM leaves the handle usable) are those of the
 * soccer_wolf_phc_* calls.  Not offered: a league or fixed-per-lane opponent, a choice of bootstrap. */
typedef struct soccer_regret_learner soccer_regret_learner;
typedef struct soccer_regret_learner_config {
    double  discount_factor;        /* [0, 1) */
    double  alpha;                  /* initial learning rate, [0, 1] */
    double  decay;                  /* alpha's factor per learner step, (0, 1] */
    double  explor;                 /* [0, 1] probability mass a LEARN player spreads uniformly over the five actions */
    double  q_init;                 /* [-1, 1] */
    int32_t act_a;                  /* SOCCER_PHC_* : how player A acts */
    int32_t act_b;                  /* SOCCER_PHC_* : how player B acts */
    int32_t plus;                   /* 0 or 1: regret matching+ */
    int32_t linear;                 /* 0 or 1: linear averaging */
    const double* policy_a;         /* act_a == SOCCER_PHC_FIXED: HOST [n_states][5] rows >= 0 summing to 1; else NULL */
    const double* policy_b;         /* the same for act_b */
} soccer_regret_learner_config;
/* what soccer_regret_learner_read fills and soccer_regret_learner_load takes: HOST pointers, any may be NULL */
typedef struct soccer_regret_learner_state {
    double* Q_a; double* Q_b;       /* [n_states][5] */
    double* R_a; double* R_b;       /* [n_states][5] */
    double* Z_a; double* Z_b;       /* [n_states][5] */
    uint64_t* visits;               /* [n_states][25] */
    uint64_t* updates;              /* [n_states] */
    double* alpha;                  /* one value */
    uint64_t* steps;
} soccer_regret_learner_state;
int soccer_regret_learner_create(soccer_handle* h, const soccer_regret_learner_config* cfg, soccer_regret_learner** out);
int soccer_regret_learner_destroy(soccer_handle* h, soccer_regret_learner* q);
/* n_steps learner steps, two launches each, enqueued on the handle's stream: no synchronisation, no copy.  Consumes n_steps ticks. */
int soccer_regret_learner_run(soccer_handle* h, soccer_regret_learner* q, int32_t n_steps);
/* steps 3-6 on the caller's batch of n <= 2^22 transitions (DEVICE pointers; reward is player A's), with the checks and the
 * misuse flags of soccer_minimax_q_update.  Consumes no tick. */
int soccer_regret_learner_update(soccer_handle* h, soccer_regret_learner* q, int64_t n, const uint16_t* obs, const int8_t* act_a,
                                 const int8_t* act_b, const int8_t* reward, const uint8_t* terminated, const uint16_t* next_obs);
/* Fills every array `out` points to (R and Z of a player that does not learn are zeros).  Synchronises. */
int soccer_regret_learner_read(soccer_handle* h, soccer_regret_learner* q, const soccer_regret_learner_state* out);
/* Resume from a checkpoint; nothing of `in` is written.  Q_a / Q_b are required, in [-1, 1].  R_p / Z_p of a LEARN player: R
 * finite, and >= 0 under `plus`; Z finite and >= 0 (SOCCER_E_INVALID, the message names array, state and action); NULL = left
 * as it is; those of a player that does not LEARN are ignored.  Row 0 of all six tables is taken as zeros.  visits / updates:
 * NULL = the counts are zeroed.  alpha (in [0, 1]) and steps: NULL = unchanged.  Everything is checked before anything is
 * written: a refused load changes nothing.  Every derived row is recomputed, so read -> load on a fresh learner continues bit
 * for bit. */
int soccer_regret_learner_load(soccer_handle* h, soccer_regret_learner* q, const soccer_regret_learner_state* in);

/* HOST output: prob[c*3+k] = slip-combination weight c (0: no slip, 1: B slips, 2: A slips,
 * 3: both; :211-222, evaluated left to right in float64) times outcome probability 1, 0.5, 0.25
 * (k = 0,1,2; :326-360).  prob_code values index this table (:241). */
int soccer_prob_table(const soccer_handle* h, double prob[12]);

/* ---- episode statistics ------------------------------------------------------------------ */
/* hist[0..2] = episodes finished with A's return -1, 0, +1 since create / soccer_reset_stats, counted by
 * batched_rollout and — on handles created with SOCCER_F_STEP_STATS — by batched_step;
 * misuse = sticky flags: SOCCER_MISUSE_FROZEN if any lane was stepped while it needed reset (the reference's
 * assert, :376; such lanes are left untouched), SOCCER_MISUSE_ACTION if any action byte on a device-pointer
 * path was outside 0..4 (the reference raises IndexError, :393; see "action bytes" above), SOCCER_MISUSE_OBSERVATION
 * if soccer_minimax_q_update was handed a transition whose observation indices no lane can be in.
 * Synchronises the stream. HOST outputs. */
#define SOCCER_MISUSE_FROZEN 1u
#define SOCCER_MISUSE_ACTION 2u
#define SOCCER_MISUSE_OBSERVATION 4u
int soccer_get_stats(soccer_handle* h, uint64_t hist[3], uint64_t* misuse);
/* caller-supplied uniforms on a slip_prob > 0 handle (batched_step_ex with u_step): the byte-parallel step decides them in
 * float64 against the slip list's nominal thresholds and leaves each 4-lane group with a uniform within 2^-40 of one (or at /
 * beyond the last) to an exact walk, one small extra launch per launch part.  parts = such launches, groups = groups they
 * walked, since create (0, 0 before the first).  Diagnostics for tests; synchronises the stream. HOST outputs (nullable). */
int soccer_exact_walk_stats(const soccer_handle* h, uint64_t* parts, uint64_t* groups);
/* the misuse flags as they stand, WITHOUT synchronising (the kernels write them to host-mapped memory): what the
 * launches that have completed so far have raised. */
uint32_t soccer_peek_misuse(const soccer_handle* h);
int soccer_reset_stats(soccer_handle* h);
uint64_t soccer_tick(const soccer_handle* h);
/* Checkpoint / resume.  The reference keeps (state tuple, timestep, needs_reset, RandomState) per env; here
 * the six state streams (soccer_get_state / soccer_set_state) plus (seed, tick) determine every later
 * result of a handle, on any device count. */
uint64_t soccer_get_seed(const soccer_handle* h);
int soccer_set_tick(soccer_handle* h, uint64_t tick);

/* Episode returns from [n_steps][n_lanes] result trajectories — what n_steps batched_step calls or one batched_rollout
 * wrote (DEVICE pointers, row stride `stride` elements): one pass over the three streams.
 *   last_return[i]   (nullable, device int8[n])  player A's return of lane i's most recently finished episode = the reward
 *                    of the last step at which terminated | truncated was set (:235-240, :400-404); 0 if none finished
 *   episode_count[i] (nullable, device int32[n]) episodes lane i finished during the n_steps steps
 *   hist             (nullable, HOST uint64[3])  all finished episodes by A's return -1, 0, +1; when given the call synchronises
 * This is the per-lane value BASELINE configs[3] gathers across GPUs (soccer_comm_all_gather). */
int soccer_trajectory_returns(soccer_handle* h, int32_t n_steps, const int8_t* reward, const uint8_t* terminated,
                              const uint8_t* truncated, int64_t stride, int8_t* last_return,
                              int32_t* episode_count, uint64_t hist[3]);

/* ---- multi-GPU: RCCL over xGMI (the reference has no counterpart) ------------------------------------
 * One process and one handle per GPU; lanes never interact, so stepping needs NO collective.  The only exchange is after a
 * run: an all-gather of per-lane episode returns into global lane order and small reductions (the 3-bin histogram, clocks).
 * librccl is resolved at run time (dlopen), so a single-GPU process never loads it.
 *   soccer_comm_unique_id   rank 0 creates the 128-byte id (ncclGetUniqueId) and hands it to every rank by any host channel
 *                           (gym_soccer_littman94_amd/comm.py: a file next to the launcher, or the caller's own)
 *   soccer_comm_init        ncclCommInitRank on the handle's device; collective over all `world` ranks
 *   soccer_comm_all_gather  recv[r * bytes_per_rank ...] = rank r's send[0 .. bytes_per_rank) (DEVICE pointers; enqueued on
 *                           the handle's stream, asynchronous): equal contiguous shards land in global lane order
 *   soccer_comm_sum_u64 / soccer_comm_max_f64 / soccer_comm_barrier   1..8 HOST values reduced over the ranks in place;
 *                           these synchronise the stream (the barrier is a one-element sum) */
#define SOCCER_COMM_ID_BYTES 128
int soccer_comm_unique_id(uint8_t id[SOCCER_COMM_ID_BYTES]);
int soccer_comm_init(soccer_handle* h, int32_t world, int32_t rank, const uint8_t id[SOCCER_COMM_ID_BYTES]);
int soccer_comm_destroy(soccer_handle* h);
int soccer_comm_all_gather(soccer_handle* h, const void* send, void* recv, uint64_t bytes_per_rank);
int soccer_comm_sum_u64(soccer_handle* h, uint64_t* values, int32_t count);
int soccer_comm_max_f64(soccer_handle* h, double* values, int32_t count);
int soccer_comm_barrier(soccer_handle* h);

/* ---- device memory + timing helpers (so a host without torch can drive the library) ------ */
int soccer_malloc(soccer_handle* h, size_t bytes, void** dptr);
int soccer_free(soccer_handle* h, void* dptr);
int soccer_memcpy_h2d(soccer_handle* h, void* dst, const void* src, size_t bytes); /* sync */
int soccer_memcpy_d2h(soccer_handle* h, void* dst, const void* src, size_t bytes); /* sync */
int soccer_memset(soccer_handle* h, void* dst, int value, size_t bytes);           /* async */
/* HIP events on the handle's stream.  soccer_timer_start / soccer_timer_mark may also be called during a graph
 * capture: the two event records then become nodes of the graph, and after a replay soccer_timer_read returns the
 * device time between them — first captured kernel's start to last one's end, without the replay's start-up latency. */
int soccer_timer_start(soccer_handle* h);
int soccer_timer_mark(soccer_handle* h);                       /* records the closing event */
int soccer_timer_read(soccer_handle* h, float* elapsed_ms);    /* waits for the closing event */
int soccer_timer_stop(soccer_handle* h, float* elapsed_ms);    /* = mark + read */
/* Device clock stamps.  soccer_stamp enqueues — or, inside a capture, records as a graph node — a one-thread kernel that
 * stores the device's constant-rate wall clock into slot `slot` of a host-mapped block; soccer_stamps_read copies slots
 * as they stand, WITHOUT synchronising (a slot reads 0 until its kernel has run, provided soccer_stamps_clear zeroed it
 * while nothing was writing it — but a line the host has just written costs the device a coherence round trip to write:
 * prefer reading the slots after a synchronisation and never clearing them) and reports the clock rate.  Every slot has a
 * 64-byte line of its own.  A captured soccer_timer_start / _mark pair is stamps 0 and 1, and after a single replay
 * soccer_timer_read just watches slot 1 change from the host: no runtime call sits between the end of the region on the
 * device and the host noticing it. */
#define SOCCER_STAMP_SLOTS 256
int soccer_stamp(soccer_handle* h, int32_t slot);
int soccer_stamps_clear(soccer_handle* h, int32_t first, int32_t count);
int soccer_stamps_read(soccer_handle* h, int32_t first, int32_t count, uint64_t* ticks, int32_t* khz);

/* ---- hipGraph capture of a sequence of batched_* calls ------------------------------------ */
/* Calls between begin and end are recorded instead of executed.  Any number of batched_* calls may be recorded (the tick
 * lives in device memory in two alternating slots so that a replay advances it; a sequence with an ODD number of recorded
 * launches gets one extra one-thread node that moves it back to the slot a replay starts from, ~1.5 us per replay).
 *
 * Deferred steps.  A captured sequence is declared before any of it runs, so the library may record it in any way that
 * leaves every output, the state, the tick and the sticky flags as one launch per call would have.  During a capture
 * batched_step / batched_step_ex check their arguments as always, but a step that qualifies is not recorded at once: it
 * joins a pending RUN, and a run of L >= 2 steps is recorded as ONE multi-step launch, the byte-parallel kernel of
 * batched_rollout with n_steps = L (no kernel boundary and no round trip of the resident state between the steps of the
 * run; bit-identical results, see soccer_rollout_args).  A run of one step is recorded exactly as before.
 *   A step qualifies when the handle created its own stream (on a caller's stream, work the caller put between two calls
 *   would be reordered) and has no fixed policy, n_lanes is a multiple of 4, the step passes no u_step / u_reset /
 *   reward_*_f32 / finished / last_return / prob_code / final_obs, and its streams are dword-aligned (obs: 8 bytes): alone
 *   it would run the byte-parallel step kernel, and a rollout over its streams the byte-parallel rollout kernel.
 *   A step extends the pending run when the same streams are NULL / non-NULL as in the run's first step and its rows
 *   continue the run's spacing: the run's second step fixes one action stride (the same for act_a and act_b) and one
 *   output stride in elements (the same for every non-NULL output), both >= n_lanes and multiples of 4.  Steps that pass
 *   the same buffers again (stride 0) never form a run.  Over the run's length no result stream may overlap another stream
 *   of the run (the two action streams are only read and may interleave, as the rows of a [T][2][n] block do).
 *   The pending run is recorded, in call order, when a step arrives that does not extend it, when any other call that may
 *   record work is made (batched_rollout*, batched_reset, soccer_stamp, soccer_timer_start / _mark, soccer_memset,
 *   soccer_reset_stats) and by soccer_graph_end.
 * Error timing: an error that only the launch can produce is returned by the call that records the run — a later step,
 * one of the calls above or soccer_graph_end — not by the step's own call.  When soccer_graph_end fails that way the
 * capture is abandoned.  A capture that is never ended, and soccer_destroy, drop the pending run.
 * SOCCER_GRAPH_FUSE=0 in the environment of soccer_create turns deferral off: every captured step is a launch.
 *
 * soccer_graph_info reports how a capture was recorded (any pointer may be NULL): kernel_nodes, the kernel nodes the
 * batched_* calls recorded (the parts of a split launch one by one; not the clock stamps, not the tick-move node);
 * steps_fused, the captured steps that went into multi-step launches; fused_launches, the runs they formed. */
int soccer_graph_begin(soccer_handle* h);
int soccer_graph_end(soccer_handle* h, soccer_graph** out);
int soccer_graph_launch(soccer_handle* h, soccer_graph* g, int32_t replays);
int soccer_graph_info(const soccer_graph* g, int32_t* kernel_nodes, int64_t* steps_fused, int32_t* fused_launches);
int soccer_graph_destroy(soccer_handle* h, soccer_graph* g);

#ifdef __cplusplus
}
#endif
#endif /* SOCCER_HIP_H */
