"""SoccerBatch — object wrapper over one libsoccer_hip handle (N lanes resident on one MI355X).

This is the thin host layer between the gym-style classes (env.py, vector_env.py) and the C ABI.
It never computes a transition itself: every step/reset is a kernel launch in libsoccer_hip.so.
"""
import ctypes as C
import weakref

import numpy as np

from . import _lib
from ._device import DeviceArray, _ptr
from ._lib import Config, RolloutArgs, StepArgs
from .learners import (GradientPlay, MinimaxQLearner, MinimaxQPopulation, OpponentModelPopulation, QLearner, QPopulation,  # noqa: F401
                       RegretLearner, RegretPopulation, WolfPHCLearner, WolfPopulation, _meta_of_cross_play, league_config,
                       minimax_q_config, minimax_q_population_config, om_derive, om_model, om_population_config, q_learning_config,
                       q_population_config, regret_average, regret_learner_config, regret_policy, regret_population_config,
                       wolf_phc_config, wolf_population_config)


def meta_lds_bytes(n_a, n_b):
    """The LDS a workgroup of the meta-game's LDS kernel takes for an n_a x n_b game (include/soccer_hip.h, "the meta-game"):
    path=1 of solve_meta_game needs this to be at most the device's limit, 163 840 bytes on gfx950."""
    stride = (n_a + n_b + 2) | 1
    return 128 + 8 * ((n_a + 2) * stride + n_a + 1) + 4 * n_a


class SoccerBatch:
    """N lanes of the Littman-94 soccer game resident on one GPU.

    Constructor arguments mirror SoccerSimultaneousEnv.__init__
    (gym_soccer/envs/soccer_simultaneous_env.py:35); failed validations raise AssertionError as the
    reference's asserts do (:45-46).
    """

    def __init__(self, n_lanes, width=5, height=4, slip_prob=0.0, seed=0, autoreset=False,
                 max_steps=100, device=0, lane_offset=0, stream=None, envs_per_thread=0, host_mapped=False, step_stats=True,
                 stream_actions=False):
        """step_stats: batched_step also feeds the episode histogram (~5 % of a launch; on by default here,
        off in the raw C ABI).
        stream_actions: batched_step reads its action streams with the non-temporal hint (SOCCER_F_STREAM_ACTIONS: action data
        that is walked through once and does not fit the Infinity Cache).
        stream: None -> the handle creates its own HIP stream; an integer hipStream_t -> enqueue on
        that stream (0 = the device's default/null stream, which is what torch's default stream is)."""
        self.lib = _lib.load()
        self.h = None
        self._arrays = weakref.WeakSet()        # device buffers handed out by alloc(); freed with the handle
        self._learners = weakref.WeakSet()      # minimax_q(), q_learning(), wolf_phc() and the populations: their memory goes with the handle
        cfg = Config(n_lanes=int(n_lanes), width=int(width), height=int(height),
                     slip_prob=float(slip_prob), max_steps=int(max_steps), device=int(device),
                     seed=int(seed) & 0xFFFFFFFFFFFFFFFF, lane_offset=int(lane_offset),
                     flags=(_lib.F_AUTORESET if autoreset else 0) | (_lib.F_NULL_STREAM if stream == 0 else 0) |
                     (_lib.F_HOST_MAPPED if host_mapped else 0) | (_lib.F_STEP_STATS if step_stats else 0) |
                     (_lib.F_STREAM_ACTIONS if stream_actions else 0),
                     envs_per_thread=int(envs_per_thread), stream=stream or None)
        h = C.c_void_p()
        _lib.check(self.lib, None, self.lib.soccer_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self.n = int(n_lanes)
        self.width, self.height, self.slip_prob = int(width), int(height), float(slip_prob)
        self.autoreset, self.max_steps = bool(autoreset), int(max_steps)
        self.device, self.lane_offset = int(device), int(lane_offset)
        ns, ll, ni, iw = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.lib.soccer_dims(self.h, C.byref(ns), C.byref(ll), C.byref(ni), C.byref(iw)))
        self.nS, self.lut_len, self.n_isd, self.internal_width = ns.value, ll.value, ni.value, iw.value
        self.nA = 5
        pt = (C.c_double * 12)()
        self._check(self.lib.soccer_prob_table(self.h, C.byref(pt)))
        self.prob_table = np.array(pt, dtype=np.float64)

    # -- plumbing -------------------------------------------------------------------------------
    def _check(self, code):
        _lib.check(self.lib, self.h, code)

    def _checked(self, code, out):
        """`out` if the call succeeded; a RuntimeError (not converged, stopped at a cap, or a capture) takes what was reached
        with it as its .results"""
        try:
            self._check(code)
        except RuntimeError as e:
            e.results = out
            raise
        return out

    def close(self):
        if self.h:
            for a in list(self._arrays):            # buffers that outlived their users: no leak past the handle
                a.free()
            for q in list(self._learners):          # soccer_destroy frees them: their wrappers must not touch them again
                q.q = None
            self.lib.soccer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def alloc(self, shape, dtype):
        a = DeviceArray(self, shape, dtype)
        self._arrays.add(a)
        return a

    def sync(self):
        self._check(self.lib.soccer_sync(self.h))

    def seed(self, seed):
        self._check(self.lib.soccer_seed(self.h, int(seed) & 0xFFFFFFFFFFFFFFFF))

    @property
    def tick(self):
        return int(self.lib.soccer_tick(self.h))

    # -- checkpoint / resume ---------------------------------------------------------------------
    def checkpoint(self):
        """Everything that determines the handle's future: the state streams, the Philox seed and the tick."""
        ck = self.get_state()
        ck["seed"] = int(self.lib.soccer_get_seed(self.h)); ck["tick"] = self.tick
        ck["rng_abi"] = int(self.lib.soccer_abi_version())      # the bits -> uniform convention the (seed, tick) pair is meant for
        return ck

    def restore(self, ck):
        """Raises AssertionError for a checkpoint taken under another RNG convention (include/soccer_hip.h, SOCCER_ABI_VERSION:
        ABI 3 changed the bits -> uniform mapping, so the same (seed, tick) would continue on a different random stream); a
        checkpoint without the field predates ABI 3's field and is refused for the same reason."""
        abi = int(self.lib.soccer_abi_version())
        assert ck.get("rng_abi") == abi, \
            "checkpoint was taken under RNG ABI %r, this library is ABI %d: resuming would silently change the random stream" % (ck.get("rng_abi"), abi)
        self.set_state(ck["row_a"], ck["col_a"], ck["row_b"], ck["col_b"], ck["poss"], t=ck["t"],
                       needs_reset=ck["needs_reset"])
        self.seed(ck["seed"])
        self._check(self.lib.soccer_set_tick(self.h, int(ck["tick"])))

    # -- tables ---------------------------------------------------------------------------------
    def tables(self):
        lut = np.zeros(self.lut_len, np.uint16)
        goal_value = np.zeros(self.lut_len, np.int8)
        isd = np.zeros((self.n_isd, 5), np.int8)
        self._check(self.lib.soccer_get_tables(self.h, lut.ctypes.data, goal_value.ctypes.data, isd.ctypes.data))
        return lut, goal_value, isd

    def transitions(self):
        """The full transition relation (the reference's P_readable), enumerated on the device.
        Returns count[T,25] (-1: unreachable tuple), prob[T,25,36], next_flat[T,25,36], reward, done."""
        T = self.lut_len
        count = np.zeros((T, 25), np.int32); prob = np.zeros((T, 25, 36), np.float64)
        nxt = np.zeros((T, 25, 36), np.int32); rew = np.zeros((T, 25, 36), np.int8); done = np.zeros((T, 25, 36), np.uint8)
        self._check(self.lib.soccer_enumerate_transitions(self.h, count.ctypes.data, prob.ctypes.data,
                                                          nxt.ctypes.data, rew.ctypes.data, done.ctypes.data))
        return count, prob, nxt, rew, done

    # -- one environment, lowest latency (n_lanes == 1) ------------------------------------------------
    def step_scalar(self, state, act_a, act_b, u_step, t=0, u_reset=0.0):
        """soccer_step_scalar: (row_a, col_a, row_b, col_b, poss), actions, uniform -> dict with the next
        tuple, t, needs_reset, obs, reward, terminated, truncated, prob_code."""
        io = _lib.ScalarIO()
        io.row_a, io.col_a, io.row_b, io.col_b, io.poss = (int(x) for x in state)
        io.t = int(t); io.act_a = int(act_a or 0); io.act_b = int(act_b or 0)
        io.u_step = float(u_step); io.u_reset = float(u_reset)
        self._check(self.lib.soccer_step_scalar(self.h, C.byref(io)))
        return self._scalar_out(io)

    def reset_scalar(self, u_reset):
        io = _lib.ScalarIO()
        io.u_reset = float(u_reset)
        self._check(self.lib.soccer_reset_scalar(self.h, C.byref(io)))
        return self._scalar_out(io)

    @staticmethod
    def _scalar_out(io):
        return {"state": (io.row_a, io.col_a, io.row_b, io.col_b, io.poss), "t": io.t, "needs_reset": io.needs_reset,
                "obs": io.obs, "reward": io.reward, "terminated": io.terminated, "truncated": io.truncated,
                "prob_code": io.prob_code}

    # -- planners on the device (single-agent mode; reference utils/planners.py) ------------------
    def _plan_out(self):
        return (np.zeros(self.nS, np.float64), np.zeros((self.nS, 5), np.float64), np.zeros(self.nS, np.int32), C.c_int32())

    def value_iteration(self, theta, discount_factor, max_sweeps=1000000):
        """Best response of the learner against the handle's fixed policy.  Returns (pi, V, Q, iterations)
        like the reference's planners.value_iteration, bit for bit."""
        V, Q, pi, it = self._plan_out()
        self._check(self.lib.soccer_value_iteration(self.h, float(theta), float(discount_factor), int(max_sweeps),
                                                    V.ctypes.data, Q.ctypes.data, pi.ctypes.data, C.byref(it)))
        return pi.astype(np.int64), V, Q, int(it.value)

    def policy_evaluation(self, pi, theta, discount_factor, max_sweeps=1000000):
        pi = np.ascontiguousarray(np.asarray(pi).reshape(-1), np.int32)
        assert pi.shape == (self.nS,), "pi must have one action per observation index"
        V, _, _, it = self._plan_out()
        self._check(self.lib.soccer_policy_evaluation(self.h, pi.ctypes.data, float(theta), float(discount_factor),
                                                      int(max_sweeps), V.ctypes.data, C.byref(it)))
        return V, int(it.value)

    def policy_improvement(self, V, discount_factor):
        V = np.ascontiguousarray(np.asarray(V).reshape(-1), np.float64)
        assert V.shape == (self.nS,), "V must have one value per observation index"
        _, Q, pi, _ = self._plan_out()
        self._check(self.lib.soccer_policy_improvement(self.h, V.ctypes.data, float(discount_factor), Q.ctypes.data, pi.ctypes.data))
        return pi.astype(np.int64), Q

    def policy_iteration(self, pi0, theta, discount_factor, max_sweeps=1000000):
        pi0 = np.ascontiguousarray(np.asarray(pi0).reshape(-1), np.int32)
        assert pi0.shape == (self.nS,), "the initial policy must have one action per observation index"
        V, Q, pi, it = self._plan_out()
        self._check(self.lib.soccer_policy_iteration(self.h, pi0.ctypes.data, float(theta), float(discount_factor),
                                                     int(max_sweeps), V.ctypes.data, Q.ctypes.data, pi.ctypes.data, C.byref(it)))
        return pi.astype(np.int64), V, Q, int(it.value)

    def policy_eval_dense(self, policy, theta, discount_factor, k=10000000, init=None, max_sweeps=10000000):
        policy = np.ascontiguousarray(policy, np.float64)
        assert policy.shape == (self.nS, 5), "policy must be [nS, nA]"
        init_p = None
        if init is not None:
            init = np.ascontiguousarray(np.asarray(init).reshape(-1), np.float64)
            assert init.shape == (self.nS,)
            init_p = init.ctypes.data
        V, _, _, it = self._plan_out()
        self._check(self.lib.soccer_policy_eval_dense(self.h, policy.ctypes.data, int(min(k, 2**31 - 1)), float(theta),
                                                      float(discount_factor), int(max_sweeps), init_p, V.ctypes.data, C.byref(it)))
        return V, int(it.value)

    def modified_policy_iteration(self, k, theta, discount_factor, max_sweeps=10000000):
        V, Q, pi, it = self._plan_out()
        self._check(self.lib.soccer_modified_policy_iteration(self.h, int(min(k, 2**31 - 1)), float(theta), float(discount_factor),
                                                              int(max_sweeps), V.ctypes.data, Q.ctypes.data, pi.ctypes.data, C.byref(it)))
        return pi.astype(np.int64), V, Q, int(it.value)

    # -- minimax planners on the device (two-player handles; Shapley's value iteration) ------------
    def solve_matrix_games(self, A):
        """A[n, 5, 5] zero-sum games (row player's payoff) -> (value[n], x[n, 5] maximin of the row player,
        y[n, 5] minimax of the column player), solved on the device; every result carries the eps certificate of
        include/soccer_hip.h."""
        A = np.ascontiguousarray(A, np.float64)
        assert A.ndim == 3 and A.shape[1:] == (5, 5), "A must be [n, 5, 5]"
        n = A.shape[0]
        v = np.zeros(n, np.float64); x = np.zeros((n, 5), np.float64); y = np.zeros((n, 5), np.float64)
        self._check(self.lib.soccer_solve_matrix_games(self.h, n, A.ctypes.data, v.ctypes.data, x.ctypes.data, y.ctypes.data))
        return v, x, y

    def _minimax_out(self):
        return (np.zeros((self.nS, 5), np.float64), np.zeros((self.nS, 5), np.float64), np.zeros(self.nS, np.float64),
                np.zeros((self.nS, 5, 5), np.float64))

    def minimax_backup(self, V, discount_factor):
        """One Shapley operator application from V: (pi_a[nS, 5], pi_b[nS, 5], V' = val(Q(V)), Q[nS, 5, 5], 1)."""
        V = np.ascontiguousarray(np.asarray(V).reshape(-1), np.float64)
        assert V.shape == (self.nS,), "V must have one value per observation index"
        pa, pb, Vo, Q = self._minimax_out()
        self._check(self.lib.soccer_minimax_backup(self.h, float(discount_factor), V.ctypes.data, Vo.ctypes.data, Q.ctypes.data,
                                                   pa.ctypes.data, pb.ctypes.data))
        return pa, pb, Vo, Q, 1

    def minimax_value_iteration(self, theta, discount_factor, max_sweeps=1000000):
        """Minimax value iteration from V = 0 until max|V_k - V_{k-1}| < theta: (pi_a[nS, 5], pi_b[nS, 5], V_k,
        Q_k[nS, 5, 5], k), with V_k = val(Q_k) and the strategies those of Q_k.  RuntimeError if max_sweeps is reached (its
        .results holds the tuple of sweep max_sweeps, which the library has copied out before it fails; a RuntimeError for
        another reason, such as a graph capture, carries a .results too, which then means nothing)."""
        pa, pb, V, Q = self._minimax_out()
        it = C.c_int32()
        code = self.lib.soccer_minimax_value_iteration(self.h, float(theta), float(discount_factor), int(max_sweeps),
                                                       V.ctypes.data, Q.ctypes.data, pa.ctypes.data, pb.ctypes.data, C.byref(it))
        return self._checked(code, (pa, pb, V, Q, int(it.value)))

    # -- best responses to mixed policies (two-player handles) ----------------------------------------
    def _policies(self, policy, name):
        """[nS, 5] or [P, nS, 5] -> (contiguous float64 [P, nS, 5], whether a leading axis was given)"""
        p = np.ascontiguousarray(policy, np.float64)
        assert p.ndim in (2, 3) and p.shape[-2:] == (self.nS, 5), "%s must be [n_states, 5] or [P, n_states, 5]" % name
        return (p if p.ndim == 3 else p[None]), p.ndim == 3

    def _policy_sets(self, pi_a, pi_b):
        """the two sets of a pair evaluator: (pi_a [n_a, nS, 5], pi_b [n_b, nS, 5], n_a, n_b)"""
        a, b = self._policies(pi_a, "pi_a")[0], self._policies(pi_b, "pi_b")[0]
        return a, b, a.shape[0], b.shape[0]

    def _response_result(self, code, out, batched):
        return self._checked(code, tuple(x if batched else x[0] for x in out[:-1]) +
                             (out[-1].astype(np.int64) if batched else int(out[-1][0]),))

    def best_response(self, policy, player, theta, discount_factor, max_sweeps=1000000):
        """The best response to a mixed policy of `player` (0: the policy is player A's and B answers, minimising; 1: it is
        B's and A answers, maximising), by value iteration from V = 0 until max|V_k - V_{k-1}| < theta.  policy is
        [nS, 5], or [P, nS, 5] for P <= 256 policies solved in one batch, each to the bits and the sweep count it has alone.
        Returns (br, V, Qr, iterations) like value_iteration: the answering side's action per state (the first optimum),
        player A's value V = the policy's worst case, Qr[.., nS, 5] per action of the answering side; with a leading axis
        only if one was given.  RuntimeError if max_sweeps is reached (its .results holds the tuple, iterations ==
        max_sweeps marks the policies that had not converged)."""
        assert player in (0, 1), "player must be 0 (the policy is player A's) or 1 (player B's)"
        p, batched = self._policies(policy, "policy")
        n = p.shape[0]
        V = np.zeros((n, self.nS)); Qr = np.zeros((n, self.nS, 5)); br = np.zeros((n, self.nS), np.int32); it = np.zeros(n, np.int32)
        code = self.lib.soccer_best_response(self.h, int(player), n, p.ctypes.data, float(theta), float(discount_factor),
                                             int(max_sweeps), V.ctypes.data, Qr.ctypes.data, br.ctypes.data, it.ctypes.data)
        return self._response_result(code, (br.astype(np.int64), V, Qr, it), batched)

    def evaluate_policies(self, pi_a, pi_b, theta, discount_factor, max_sweeps=1000000):
        """Player A's value of the pair (pi_a, pi_b) of mixed policies, iterated like best_response: (V, iterations).
        [nS, 5] each, or [P, nS, 5] (one of them may be a single policy: it meets every policy of the other)."""
        a, b, na, nb = self._policy_sets(pi_a, pi_b)
        n = max(na, nb)
        assert na in (1, n) and nb in (1, n), "pi_a and pi_b must hold one policy or the same number of policies"
        a = np.ascontiguousarray(np.broadcast_to(a, (n, self.nS, 5))); b = np.ascontiguousarray(np.broadcast_to(b, (n, self.nS, 5)))
        V = np.zeros((n, self.nS)); it = np.zeros(n, np.int32)
        code = self.lib.soccer_evaluate_policies(self.h, n, a.ctypes.data, b.ctypes.data, float(theta), float(discount_factor),
                                                 int(max_sweeps), V.ctypes.data, it.ctypes.data)
        return self._response_result(code, (V, it), np.ndim(pi_a) == 3 or np.ndim(pi_b) == 3)

    def cross_play(self, pi_a, pi_b, theta, discount_factor, max_sweeps=1000000, pairs_per_pass=0, values=False):
        """The payoff matrix of two sets of mixed policies: payoff[i, j] is player A's value at kick-off (the mean of V over the
        initial states) when pi_a[i] meets pi_b[j], each pair iterated exactly like evaluate_policies on that pair alone.
        pi_a is [n_a, nS, 5], pi_b [n_b, nS, 5], up to 1024 policies each (a single [nS, 5] policy is a batch of one).
        Returns (payoff[n_a, n_b], iterations[n_a, n_b]), and with values=True also V[n_a, n_b, nS].  pairs_per_pass: how many
        pairs are solved together on the device (0: the library chooses; else a multiple of 64) — no result depends on it.
        RuntimeError if max_sweeps is reached (its .results holds the tuple, iterations == max_sweeps marks the open pairs)."""
        a, b, na, nb = self._policy_sets(pi_a, pi_b)
        payoff = np.zeros((na, nb)); it = np.zeros((na, nb), np.int32)
        V = np.zeros((na, nb, self.nS)) if values else None
        code = self.lib.soccer_cross_play(self.h, na, a.ctypes.data, nb, b.ctypes.data, float(theta), float(discount_factor),
                                          int(max_sweeps), int(pairs_per_pass), payoff.ctypes.data,
                                          V.ctypes.data if values else None, it.ctypes.data)
        return self._checked(code, (payoff, it.astype(np.int64)) + ((V,) if values else ()))

    def match_outcomes(self, pi_a, pi_b, theta, continue_prob, max_sweeps=1000000, pairs_per_pass=0, values=False):
        """Littman's columns for two sets of mixed policies, exactly (include/soccer_hip.h, "match outcomes"): after every step
        the game goes on with probability continue_prob and is a draw otherwise.  pi_a, pi_b, pairs_per_pass and the limits are
        cross_play's.  Returns a dict of [n_a, n_b] arrays at kick-off, pi_a[i] against pi_b[j]:
          win_a, win_b    the probability that A's side, B's side scores the goal that ends the game
          draw            1.0 - win_a - win_b
          length          the expected number of steps of a game,  games_per_step  1 / length
          iterations      the sweeps of each pair's solve (int64)
          values          [n_a, n_b, 3, nS] with values=True: W_A, W_B and L at every state
        RuntimeError if max_sweeps is reached (its .results holds the dict, iterations == max_sweeps marks the open pairs,
        which hold the max_sweeps-step numbers)."""
        a, b, na, nb = self._policy_sets(pi_a, pi_b)
        win_a = np.zeros((na, nb)); win_b = np.zeros((na, nb)); length = np.zeros((na, nb)); it = np.zeros((na, nb), np.int32)
        V = np.zeros((na, nb, 3, self.nS)) if values else None
        code = self.lib.soccer_match_outcomes(self.h, na, a.ctypes.data, nb, b.ctypes.data, float(theta), float(continue_prob),
                                              int(max_sweeps), int(pairs_per_pass), win_a.ctypes.data, win_b.ctypes.data,
                                              length.ctypes.data, V.ctypes.data if values else None, it.ctypes.data)
        with np.errstate(divide="ignore"):
            out = {"win_a": win_a, "win_b": win_b, "draw": 1.0 - win_a - win_b, "length": length, "games_per_step": 1.0 / length,
                   "iterations": it.astype(np.int64)}
        if values:
            out["values"] = V
        return self._checked(code, out)

    def occupancy(self, pi_a, pi_b, theta, continue_prob, features=None, values=False, max_sweeps=1000000, pairs_per_pass=0):
        """Where the game is played when two sets of mixed policies meet, exactly (include/soccer_hip.h, "state occupancy"): the
        expected number of visits to every state from kick-off when after every step the game goes on with probability
        continue_prob — the dual of the value.  pi_a, pi_b, pairs_per_pass and the limits are cross_play's; features is
        [n_f, nS] (or one [nS] vector), at most 16 of them.  Returns a dict, pi_a[i] against pi_b[j]:
          length          [n_a, n_b] the expected number of steps of a game, the sum of the occupancy over the states
          expect          [n_a, n_b, n_f] the sum over the states of occupancy * features[q]: with an indicator, the steps
                          spent in its states
          iterations      [n_a, n_b] the sweeps of each pair's solve (int64)
          occupancy       [n_a, n_b, nS] with values=True, and  visit_share = occupancy / length
        RuntimeError if max_sweeps is reached (its .results holds the dict, iterations == max_sweeps marks the open pairs,
        which hold the last iterate)."""
        a, b, na, nb = self._policy_sets(pi_a, pi_b)
        F = np.zeros((0, self.nS)) if features is None else np.ascontiguousarray(features, np.float64)
        F = F[None] if F.ndim == 1 else F
        assert F.ndim == 2 and F.shape[1] == self.nS, "features must be [n_f, n_states] or [n_states]"
        nf = F.shape[0]
        length = np.zeros((na, nb)); expect = np.zeros((na, nb, nf)); it = np.zeros((na, nb), np.int32)
        D = np.zeros((na, nb, self.nS)) if values else None
        code = self.lib.soccer_occupancy(self.h, na, a.ctypes.data, nb, b.ctypes.data, float(theta), float(continue_prob),
                                         int(max_sweeps), int(pairs_per_pass), nf, F.ctypes.data if nf else None, length.ctypes.data,
                                         expect.ctypes.data if nf else None, D.ctypes.data if values else None, it.ctypes.data)
        out = {"length": length, "expect": expect, "iterations": it.astype(np.int64)}
        if values:
            out["occupancy"] = D
            with np.errstate(divide="ignore", invalid="ignore"):
                out["visit_share"] = D / length[:, :, None]
        return self._checked(code, out)

    def _weights(self, w, n, name):
        if w is None:
            return None
        w = np.ascontiguousarray(w, np.float64)
        assert w.shape == (n,), "%s must hold one weight per policy (%d)" % (name, n)
        return w

    def policy_gradient(self, pi_a, pi_b, theta, discount_factor, w_a=None, w_b=None, normalize=False, values=False,
                        max_sweeps=1000000, pairs_per_pass=0):
        """The exact policy gradients of two sets of mixed policies (include/soccer_hip.h, "exact policy gradients"): under the
        direct parametrisation d payoff / d x[s][a] = D[s] * Q_a[s][a], D the discounted occupancy from kick-off and Q_a player
        A's action values against the opponent's policy.  pi_a, pi_b, pairs_per_pass and the limits are cross_play's; w_b [n_b]
        weighs the opponents of A's policies and w_a [n_a] those of B's (None: uniform).  Returns a dict:
          payoff      [n_a, n_b] cross_play's,  iterations  [n_a, n_b, 2] the sweeps of each pair's V and D solves (int64)
          grad_a      [n_a, nS, 5] the gradient of sum_j w_b[j] * payoff[i, j] in pi_a[i],  reach_a [n_a, nS] = sum_j w_b[j] D_ij
          grad_b      [n_b, nS, 5] the gradient of sum_i w_a[i] * payoff[i, j] in pi_b[j] (player A's payoff: B descends it),
                      reach_b [n_b, nS]
          q_a, q_b    [n_a, n_b, nS, 5], V and occupancy [n_a, n_b, nS], with values=True
        normalize=True divides every grad row by its reach (0 where the reach is 0).
        RuntimeError if max_sweeps is reached (its .results holds the dict, iterations == max_sweeps marks the open solves)."""
        a, b, na, nb = self._policy_sets(pi_a, pi_b)
        nS = self.nS
        wa, wb = self._weights(w_a, na, "w_a"), self._weights(w_b, nb, "w_b")
        out = {"payoff": np.zeros((na, nb)), "grad_a": np.zeros((na, nS, 5)), "grad_b": np.zeros((nb, nS, 5)),
               "reach_a": np.zeros((na, nS)), "reach_b": np.zeros((nb, nS))}
        if values:
            out.update(q_a=np.zeros((na, nb, nS, 5)), q_b=np.zeros((na, nb, nS, 5)), V=np.zeros((na, nb, nS)),
                       occupancy=np.zeros((na, nb, nS)))
        it = np.zeros((na, nb, 2), np.int32)
        ptr = [out[k].ctypes.data if k in out else None
               for k in ("payoff", "grad_a", "grad_b", "reach_a", "reach_b", "q_a", "q_b", "V", "occupancy")]
        code = self.lib.soccer_policy_gradient(self.h, na, a.ctypes.data, nb, b.ctypes.data, float(theta), float(discount_factor),
                                               int(max_sweeps), int(pairs_per_pass), None if wa is None else wa.ctypes.data,
                                               None if wb is None else wb.ctypes.data, int(bool(normalize)), *ptr, it.ctypes.data)
        out["iterations"] = it.astype(np.int64)
        return self._checked(code, out)

    def gradient_play(self, n_a=1, n_b=1, discount_factor=0.9, eta_a=1.0, eta_b=1.0, optimism=0.0, normalize=True, theta=1e-10,
                      max_sweeps=1000000, pairs_per_pass=0, pi_a=None, pi_b=None):
        """A GradientPlay on this batch (two players): n_a policies of player A and n_b of player B on the device that take
        projected steps along policy_gradient's exact gradients of themselves."""
        return GradientPlay(self, n_a, n_b, discount_factor, eta_a=eta_a, eta_b=eta_b, optimism=optimism, normalize=normalize,
                            theta=theta, max_sweeps=max_sweeps, pairs_per_pass=pairs_per_pass, pi_a=pi_a, pi_b=pi_b)

    def solve_meta_game(self, payoff, max_pivots=None, path=0, pivots_per_sync=0):
        """The maximin mixtures of zero-sum matrix games of any shape up to 1024 a side (include/soccer_hip.h, "the meta-game"):
        payoff is [n_a, n_b] or [g, n_a, n_b], the row player's (the maximiser's) payoffs, for instance cross_play's matrix.
        Returns a dict (a [g, ..] input: arrays with a leading g): x[n_a] and y[n_b] the two mixtures, lo = min_j (x @ payoff)_j
        what x guarantees, hi = max_i (payoff @ y)_i what y concedes at most, value their midpoint, gap = hi - lo, pivots,
        status (1 saddle point, 0 gap <= 1e-10 * max(1, max|payoff|), 2 finished but wider, 3 stopped at max_pivots) and
        certified = status <= 1.  lo <= the game's value <= hi holds whatever the status.  max_pivots None: 100 * (n_a + n_b).
        path: 0 the library chooses, 1 the LDS kernel (AssertionError if the game does not fit, meta_lds_bytes), 2 the global
        kernels; pivots_per_sync: 0 the library chooses — no result depends on either.
        AssertionError for an entry that is not finite and for a game whose max - min is not finite (1e308 and -1e308).
        RuntimeError if a game stopped at max_pivots (its .results holds the dict: the last basis and its valid bracket)."""
        A = np.ascontiguousarray(payoff, np.float64)
        assert A.ndim in (2, 3), "payoff must be [n_a, n_b] or [g, n_a, n_b]"
        single = A.ndim == 2
        g = 1 if single else A.shape[0]
        n_a, n_b = A.shape[-2:]
        if max_pivots is None:
            max_pivots = 100 * (n_a + n_b)
        out = {"value": np.zeros(g), "x": np.zeros((g, n_a)), "y": np.zeros((g, n_b)), "lo": np.zeros(g), "hi": np.zeros(g),
               "pivots": np.zeros(g, np.int32), "status": np.zeros(g, np.int32)}
        res = _lib.MetaGameResult(**{k: v.ctypes.data for k, v in out.items()})
        code = self.lib.soccer_solve_meta_games(self.h, g, n_a, n_b, A.ctypes.data, int(max_pivots), int(path), int(pivots_per_sync),
                                                C.byref(res))
        out["gap"] = out["hi"] - out["lo"]
        out["certified"] = out["status"] <= 1
        if single:
            out = {k: v[0] for k, v in out.items()}
        return self._checked(code, out)

    # -- learners -------------------------------------------------------------------------------
    def minimax_q(self, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, opponent="uniform"):
        """A MinimaxQLearner on this batch (two players, autoreset=True, at most 2**22 lanes).  opponent: 'uniform', 'self'
        (player B follows its own minimax strategy of the learned Q, with the same exploration) or a fixed [nS, 5] policy."""
        return MinimaxQLearner(self, discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init, opponent=opponent)

    def q_learning(self, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, act_a="greedy", act_b="greedy"):
        """A QLearner on this batch (two players, autoreset=True, at most 2**22 lanes).  act_a / act_b: 'greedy'
        (epsilon-greedy on the player's own table), 'uniform', or a fixed [nS, 5] mixed policy.  Both tables always learn."""
        return QLearner(self, discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init, act_a=act_a, act_b=act_b)

    def q_population(self, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, act_a="greedy", act_b="greedy",
                     league_policies=None, league_weights=None):
        """A QPopulation on this batch (two players, autoreset=True): a Q-learner per lane, each with its own tables.
        discount_factor, alpha, decay and explor are scalars or arrays of one value per lane; act_a / act_b as for
        q_learning (a fixed policy is shared by all members), or — one of them — "league": that player draws one of
        league_policies [K, nS, 5] with probability league_weights [K] at every kick-off and plays it to the end of the
        episode (include/soccer_hip.h, "learners, a league opponent for the population of Q-learners")."""
        return QPopulation(self, discount_factor, league_policies=league_policies, league_weights=league_weights, alpha=alpha, decay=decay,
                           explor=explor, q_init=q_init, act_a=act_a, act_b=act_b)

    def om_population(self, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, act_a="greedy", act_b="greedy"):
        """An OpponentModelPopulation on this batch (two players, autoreset=True): an opponent-modelling Q-learner per lane,
        each with its own joint-action tables and counts of the other player's actions.  discount_factor, alpha, decay and
        explor are scalars or arrays of one value per lane; act_a / act_b as for q_learning: 'greedy' answers the other
        player's empirical frequencies (a fixed policy is shared by all members)."""
        return OpponentModelPopulation(self, discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init, act_a=act_a, act_b=act_b)

    def wolf_phc(self, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, delta_win=0.01, delta_lose=0.04,
                 delta_decay=1.0, act_a="learn", act_b="learn"):
        """A WolfPHCLearner on this batch (two players, autoreset=True, at most 2**22 lanes).  act_a / act_b: 'learn'
        (a hill-climbing mixed policy), 'uniform' or a fixed [nS, 5] mixed policy; delta_win == delta_lose is plain PHC."""
        return WolfPHCLearner(self, discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init, delta_win=delta_win,
                              delta_lose=delta_lose, delta_decay=delta_decay, act_a=act_a, act_b=act_b)

    def wolf_population(self, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, delta_win=0.01, delta_lose=0.04,
                        delta_decay=1.0, act_a="learn", act_b="learn"):
        """A WolfPopulation on this batch (two players, autoreset=True): a PHC / WoLF-PHC learner per lane, each with its own
        tables and policies.  The seven hyperparameters are scalars or arrays of one value per lane; act_a / act_b: 'learn',
        'uniform', a fixed [nS, 5] mixed policy for every member or [n, nS, 5], one per member."""
        return WolfPopulation(self, discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init, delta_win=delta_win,
                              delta_lose=delta_lose, delta_decay=delta_decay, act_a=act_a, act_b=act_b)

    def minimax_q_population(self, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, opponent="uniform"):
        """A MinimaxQPopulation on this batch (two players, autoreset=True): a minimax-Q learner per lane, each with its own
        Q, V and strategies.  discount_factor, alpha, decay and explor are scalars or arrays of one value per lane; opponent:
        'uniform', 'self', a fixed [nS, 5] mixed policy for every member or [n, nS, 5], one per member."""
        return MinimaxQPopulation(self, discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init, opponent=opponent)

    def regret_population(self, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, plus=True, linear=False,
                          act_a="learn", act_b="learn"):
        """A RegretPopulation on this batch (two players, autoreset=True): a regret-matching learner per lane, each with its
        own tables, cumulative regrets and policy sums.  discount_factor, alpha, decay and explor are scalars or arrays of one
        value per lane; plus floors the regrets at 0 (regret matching+), linear weighs a step's policy by the state's visit
        count; act_a / act_b: 'learn', 'uniform', a fixed [nS, 5] mixed policy for every member or [n, nS, 5], one per
        member."""
        return RegretPopulation(self, discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init, plus=plus, linear=linear,
                                act_a=act_a, act_b=act_b)

    def regret_matching(self, discount_factor, **params):
        """A RegretLearner on this batch (two players, autoreset=True, at most 2**22 lanes): regret matchers for both players
        with one table that every lane feeds.  params: alpha, decay, explor, q_init, plus (regret matching+), linear (linear
        averaging), act_a / act_b: 'learn', 'uniform' or a fixed [nS, 5] mixed policy (learners.regret_learner_config)."""
        return RegretLearner(self, discount_factor, **params)

    # -- hot path -------------------------------------------------------------------------------
    def reset(self, mask=None, u_reset=None, obs=None):
        self._check(self.lib.batched_reset(self.h, _ptr(mask), _ptr(u_reset), _ptr(obs)))

    def step(self, act_a, act_b, obs=None, reward=None, terminated=None, truncated=None,
             prob_code=None, u_step=None, u_reset=None, final_obs=None, last_return=None,
             reward_a_f32=None, reward_b_f32=None, finished=None):
        a = StepArgs(_ptr(act_a), _ptr(act_b), _ptr(u_step), _ptr(u_reset), _ptr(obs), _ptr(reward),
                     _ptr(terminated), _ptr(truncated), _ptr(prob_code), _ptr(final_obs), _ptr(last_return),
                     _ptr(reward_a_f32), _ptr(reward_b_f32), _ptr(finished))
        self._check(self.lib.batched_step_ex(self.h, C.byref(a)))

    def step_plain(self, act_a, act_b, obs, reward, terminated, truncated, prob_code=None):
        """The 8-argument batched_step entry point (per-lane Philox)."""
        self._check(self.lib.batched_step(self.h, _ptr(act_a), _ptr(act_b), _ptr(obs), _ptr(reward),
                                          _ptr(terminated), _ptr(truncated), _ptr(prob_code)))

    def rollout(self, n_steps, act_a=None, act_b=None, act_stride=0, sample_actions=False, obs=None,
                reward=None, terminated=None, truncated=None, out_stride=0, return_sum=None,
                episode_count=None, mix_a=None, mix_b=None, final_obs=None, prob_code=None):
        """batched_rollout; with final_obs / prob_code ([T][n] like the four result trajectories) batched_rollout_ex."""
        a = RolloutArgs(int(n_steps), 1 if sample_actions else 0, _ptr(act_a), _ptr(act_b), int(act_stride),
                        _ptr(obs), _ptr(reward), _ptr(terminated), _ptr(truncated), int(out_stride),
                        _ptr(return_sum), _ptr(episode_count), _ptr(mix_a), _ptr(mix_b))
        if final_obs is None and prob_code is None:
            self._check(self.lib.batched_rollout(self.h, C.byref(a)))
        else:
            x = _lib.RolloutExtra(_ptr(final_obs), _ptr(prob_code))
            self._check(self.lib.batched_rollout_ex(self.h, C.byref(a), C.byref(x)))

    def rollout_shape(self):
        """soccer_rollout_shape: which launch shape the most recent rollout() took, as a dict of ints — kernel (0 none yet,
        1 byte-parallel, 2 per-lane), tail, action_source (0..5), slip_selection (0..2), small_pitch, full, table_placement
        (0 none, 1 LDS, 2 global memory), parts, chunks, dynamic_lds_bytes, lds_limit.  Diagnostics: results never depend on it."""
        s = _lib.RolloutShape()
        self._check(self.lib.soccer_rollout_shape(self.h, C.byref(s)))
        return {name: int(getattr(s, name)) for name, _ in s._fields_ if name != "reserved_"}

    def trajectory_returns(self, n_steps, reward, terminated, truncated, stride, last_return=None, episode_count=None, hist=True):
        """soccer_trajectory_returns: one pass over [n_steps][n] result trajectories (device) -> per-lane return of the most recently
        finished episode (int8[n]), per-lane finished-episode count (int32[n]) and, with hist=True (synchronises), the
        (-1, 0, +1) histogram of every finished episode as a uint64[3] array."""
        h3 = (C.c_uint64 * 3)() if hist else None
        self._check(self.lib.soccer_trajectory_returns(self.h, int(n_steps), _ptr(reward), _ptr(terminated), _ptr(truncated), int(stride),
                                                       _ptr(last_return), _ptr(episode_count), C.byref(h3) if hist else None))
        return np.array(h3, dtype=np.uint64) if hist else None

    # -- multi-GPU: RCCL over xGMI through the C ABI (one handle per process and GPU; see comm.py for the bring-up) -----
    def comm_init(self, world, rank, unique_id):
        assert len(unique_id) == _lib.COMM_ID_BYTES
        buf = (C.c_uint8 * _lib.COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        self._check(self.lib.soccer_comm_init(self.h, int(world), int(rank), buf))

    def comm_destroy(self):
        self._check(self.lib.soccer_comm_destroy(self.h))

    def all_gather(self, send, recv, bytes_per_rank):
        """recv[r * bytes_per_rank ...] = rank r's send[:bytes_per_rank] (device buffers; asynchronous on the handle's stream)."""
        self._check(self.lib.soccer_comm_all_gather(self.h, _ptr(send), _ptr(recv), int(bytes_per_rank)))

    def comm_sum(self, values):
        a = np.ascontiguousarray(values, np.uint64).copy()
        self._check(self.lib.soccer_comm_sum_u64(self.h, a.ctypes.data, int(a.size)))
        return a

    def comm_max(self, values):
        a = np.ascontiguousarray(values, np.float64).copy()
        self._check(self.lib.soccer_comm_max_f64(self.h, a.ctypes.data, int(a.size)))
        return a

    def comm_barrier(self):
        self._check(self.lib.soccer_comm_barrier(self.h))

    @staticmethod
    def mixed_policy_thresholds(probs):
        """[nS, 5] action probabilities -> uint16[nS, 4] cumulative thresholds for batched_rollout's
        mix_a / mix_b: floor(32768 * cumulative probability), values 0..32768; the sampled action is the
        number of thresholds <= a 15-bit draw, so deterministic rows are reproduced exactly."""
        p = np.asarray(probs, dtype=np.float64)
        assert p.ndim == 2 and p.shape[1] == 5 and (p >= 0).all() and np.allclose(p.sum(1), 1.0), \
            "probs must be [n_states, 5] rows summing to 1"
        c = np.cumsum(p, axis=1)[:, :4]
        return np.ascontiguousarray(np.clip(np.floor(c * 32768.0 + 1e-9), 0, 32768).astype(np.uint16))

    def set_policy(self, player, policy):
        """Fixed policy for 'player_a' / 'player_b' (dict or sequence: observation index -> action), or None."""
        idx = {"player_a": 0, "player_b": 1, 0: 0, 1: 1}[player]
        if policy is None:
            self._check(self.lib.soccer_set_policy(self.h, idx, None, 0)); return
        arr = np.array([policy[s] for s in range(self.nS)], dtype=np.int8) if isinstance(policy, dict) \
            else np.ascontiguousarray(policy, dtype=np.int8)
        self._check(self.lib.soccer_set_policy(self.h, idx, arr.ctypes.data, int(arr.size)))

    # -- zero-copy staged I/O: numpy views over the handle's pinned staging block ----------------
    def staging(self):
        """dict of numpy arrays (length n) over the pinned staging block: inputs act_a, act_b, mask, u_step,
        u_reset; outputs obs, final_obs, reward, terminated, truncated, prob_code (overwritten by the
        next staged call)."""
        if getattr(self, "_staging", None) is None:
            v = _lib.StagingView()
            self._check(self.lib.soccer_staging(self.h, C.byref(v)))
            def view(ptr, dt):
                dt = np.dtype(dt)
                buf = (C.c_uint8 * (self.n * dt.itemsize)).from_address(ptr)
                return np.frombuffer(buf, dtype=dt)
            self._staging = {"act_a": view(v.act_a, np.int8), "act_b": view(v.act_b, np.int8),
                             "mask": view(v.mask, np.uint8), "u_step": view(v.u_step, np.float64),
                             "u_reset": view(v.u_reset, np.float64), "obs": view(v.obs, np.uint16),
                             "final_obs": view(v.final_obs, np.uint16), "reward": view(v.reward, np.int8),
                             "terminated": view(v.terminated, np.uint8), "truncated": view(v.truncated, np.uint8),
                             "prob_code": view(v.prob_code, np.uint8)}
        return self._staging

    def step_staged(self, act_a=True, act_b=True, u_step=False, u_reset=False):
        use = (_lib.STAGE_ACT_A if act_a else 0) | (_lib.STAGE_ACT_B if act_b else 0) | \
              (_lib.STAGE_U_STEP if u_step else 0) | (_lib.STAGE_U_RESET if u_reset else 0)
        self._check(self.lib.batched_step_staged(self.h, use))

    def reset_staged(self, mask=False, u_reset=False):
        self._check(self.lib.batched_reset_staged(self.h, (_lib.STAGE_MASK if mask else 0) |
                                                  (_lib.STAGE_U_RESET if u_reset else 0)))

    # -- host-array variants (numpy in, numpy out; one staged copy each way) -------------------
    def reset_host(self, mask=None, u_reset=None):
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        u = None if u_reset is None else np.ascontiguousarray(u_reset, np.float64)
        obs = np.empty(self.n, np.uint16)
        self._check(self.lib.batched_reset_host(self.h, None if m is None else m.ctypes.data,
                                                None if u is None else u.ctypes.data, obs.ctypes.data))
        return obs

    def step_host(self, act_a, act_b, u_step=None, u_reset=None):
        n = self.n
        a = None if act_a is None else np.ascontiguousarray(act_a, np.int8)
        b = None if act_b is None else np.ascontiguousarray(act_b, np.int8)
        assert (a is None or a.shape == (n,)) and (b is None or b.shape == (n,)), \
            "actions must have one entry per environment"
        us = None if u_step is None else np.ascontiguousarray(u_step, np.float64)
        ur = None if u_reset is None else np.ascontiguousarray(u_reset, np.float64)
        out = {"obs": np.empty(n, np.uint16), "reward": np.empty(n, np.int8),
               "terminated": np.empty(n, np.uint8), "truncated": np.empty(n, np.uint8),
               "prob_code": np.empty(n, np.uint8), "final_obs": np.empty(n, np.uint16)}
        args = StepArgs(None if a is None else a.ctypes.data, None if b is None else b.ctypes.data, None if us is None else us.ctypes.data,
                        None if ur is None else ur.ctypes.data, out["obs"].ctypes.data,
                        out["reward"].ctypes.data, out["terminated"].ctypes.data,
                        out["truncated"].ctypes.data, out["prob_code"].ctypes.data,
                        out["final_obs"].ctypes.data, None)
        self._check(self.lib.batched_step_host(self.h, C.byref(args)))
        return out

    def host_state_view(self):
        """host_mapped handles: numpy uint8 view [6, n] over the pinned state streams (row_a, col_a, row_b,
        col_b, poss | needs_reset << 1, t) the GPU works on in place.  Touch it only while the stream is idle."""
        p = C.c_void_p(); stride = C.c_uint64()
        self._check(self.lib.soccer_host_view(self.h, C.byref(p), C.byref(stride)))
        buf = (C.c_uint8 * (6 * stride.value)).from_address(p.value)
        return np.frombuffer(buf, dtype=np.uint8).reshape(6, stride.value)[:, :self.n]

    def state_streams(self):
        """3 when the handle keeps its resident state packed in three byte streams, 6 otherwise (results are the same)."""
        return int(self.lib.soccer_state_streams(self.h))

    # -- state injection / readback -----------------------------------------------------------
    def set_state(self, row_a=None, col_a=None, row_b=None, col_b=None, poss=None, t=None, needs_reset=None):
        def arr(x, dt):
            if x is None:
                return None, None
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(x, dt), (self.n,)), dt)
            return a, a.ctypes.data
        keep = []
        ptrs = []
        for x, dt in ((row_a, np.int8), (col_a, np.int8), (row_b, np.int8), (col_b, np.int8),
                      (poss, np.uint8), (t, np.uint8), (needs_reset, np.uint8)):
            a, p = arr(x, dt); keep.append(a); ptrs.append(p)
        code = self.lib.soccer_set_state(self.h, *ptrs)
        if code == _lib.E_INVALID:
            msg = self.lib.soccer_last_error(self.h).decode()
            if "not a reachable state tuple" in msg:
                raise KeyError(msg)        # the reference's P_readable[self.state] lookup (:394)
        self._check(code)

    def get_state(self):
        n = self.n
        out = {k: np.zeros(n, np.int8) for k in ("row_a", "col_a", "row_b", "col_b")}
        out.update({k: np.zeros(n, np.uint8) for k in ("poss", "t", "needs_reset")})
        self._check(self.lib.soccer_get_state(self.h, *[out[k].ctypes.data for k in
                    ("row_a", "col_a", "row_b", "col_b", "poss", "t", "needs_reset")]))
        return out

    # -- statistics / timing ------------------------------------------------------------------
    def stats(self):
        hist = (C.c_uint64 * 3)(); mis = C.c_uint64()
        self._check(self.lib.soccer_get_stats(self.h, C.byref(hist), C.byref(mis)))
        return np.array(hist, dtype=np.uint64), int(mis.value)

    MISUSE_FROZEN, MISUSE_ACTION, MISUSE_OBSERVATION = 1, 2, 4

    def misuse(self):
        """The sticky misuse flags alone (no histogram copy; synchronises): MISUSE_FROZEN if a lane was stepped while
        it needed reset (:376), MISUSE_ACTION if a device-side action byte was outside 0..4 (:393)."""
        mis = C.c_uint64()
        self._check(self.lib.soccer_get_stats(self.h, None, C.byref(mis)))
        return int(mis.value)

    def exact_walk_stats(self):
        """(parts, groups): launches of the exact walk that caller-supplied uniforms on a slip list take for the 4-lane groups
        within 2^-40 of a threshold, and the groups they walked, since create (synchronises)."""
        parts = C.c_uint64(); groups = C.c_uint64()
        self._check(self.lib.soccer_exact_walk_stats(self.h, C.byref(parts), C.byref(groups)))
        return int(parts.value), int(groups.value)

    def peek_misuse(self):
        """The same flags WITHOUT synchronising: what the launches completed so far have raised."""
        return int(self.lib.soccer_peek_misuse(self.h))

    def reset_stats(self):
        self._check(self.lib.soccer_reset_stats(self.h))

    def timer_start(self):
        self._check(self.lib.soccer_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        self._check(self.lib.soccer_timer_stop(self.h, C.byref(ms)))
        return float(ms.value)

    def timer_mark(self):
        """Record the closing event (allowed inside a graph capture, like timer_start)."""
        self._check(self.lib.soccer_timer_mark(self.h))

    def timer_read(self):
        ms = C.c_float()
        self._check(self.lib.soccer_timer_read(self.h, C.byref(ms)))
        return float(ms.value)

    def stamp(self, slot):
        """Enqueue (or capture) a device clock stamp into slot 0..255 of the handle's host-mapped block."""
        self._check(self.lib.soccer_stamp(self.h, int(slot)))

    def stamps_clear(self, first=0, count=256):
        self._check(self.lib.soccer_stamps_clear(self.h, int(first), int(count)))

    def stamps(self, first=0, count=256):
        """(ticks[count] uint64, clock kHz) — the slots as they stand, no synchronisation; 0 = not written since cleared."""
        t = np.zeros(int(count), np.uint64); khz = C.c_int32()
        self._check(self.lib.soccer_stamps_read(self.h, int(first), int(count), t.ctypes.data, C.byref(khz)))
        return t, int(khz.value)

    # -- hipGraph capture ----------------------------------------------------------------------
    def graph_begin(self):
        self._check(self.lib.soccer_graph_begin(self.h))

    def graph_end(self):
        g = C.c_void_p()
        self._check(self.lib.soccer_graph_end(self.h, C.byref(g)))
        return g

    def graph_launch(self, g, replays=1):
        self._check(self.lib.soccer_graph_launch(self.h, g, int(replays)))

    def graph_info(self, g):
        """How a capture was recorded: {"kernel_nodes", "steps_fused", "fused_launches"} (soccer_graph_info)."""
        nodes, steps, runs = C.c_int32(), C.c_int64(), C.c_int32()
        self._check(self.lib.soccer_graph_info(g, C.byref(nodes), C.byref(steps), C.byref(runs)))
        return {"kernel_nodes": int(nodes.value), "steps_fused": int(steps.value), "fused_launches": int(runs.value)}

    def graph_destroy(self, g):
        self.lib.soccer_graph_destroy(self.h, g)
