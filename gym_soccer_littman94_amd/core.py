"""SoccerBatch — object wrapper over one libsoccer_hip handle (N lanes resident on one MI355X).

This is the thin host layer between the gym-style classes (env.py, vector_env.py) and the C ABI.
It never computes a transition itself: every step/reset is a kernel launch in libsoccer_hip.so.
"""
import ctypes as C
import weakref

import numpy as np

from . import _lib
from ._lib import Config, RolloutArgs, StepArgs


class DeviceArray:
    """A caller-owned device buffer allocated through the handle (no torch needed)."""

    def __init__(self, batch, shape, dtype):
        self.batch = batch
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        batch._check(batch.lib.soccer_malloc(batch.h, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, host):
        a = np.ascontiguousarray(host, dtype=self.dtype)
        assert a.nbytes == self.nbytes, "size mismatch: %d vs %d bytes" % (a.nbytes, self.nbytes)
        b = self.batch
        b._check(b.lib.soccer_memcpy_h2d(b.h, self.ptr, a.ctypes.data, self.nbytes))
        return self

    def upload_rows(self, first_row, host):
        """Copy `host` (rows of the same width) into rows first_row.. of a 2-D+ buffer."""
        a = np.ascontiguousarray(host, dtype=self.dtype)
        row_bytes = int(np.prod(self.shape[1:])) * self.dtype.itemsize
        assert a.nbytes % row_bytes == 0 and int(first_row) * row_bytes + a.nbytes <= self.nbytes
        b = self.batch
        b._check(b.lib.soccer_memcpy_h2d(b.h, self.ptr + int(first_row) * row_bytes, a.ctypes.data, a.nbytes))
        return self

    def download_rows(self, first_row, n_rows):
        row_bytes = int(np.prod(self.shape[1:])) * self.dtype.itemsize
        out = np.empty((int(n_rows),) + self.shape[1:], self.dtype)
        b = self.batch
        b._check(b.lib.soccer_memcpy_d2h(b.h, out.ctypes.data, self.ptr + int(first_row) * row_bytes, out.nbytes))
        return out

    def download(self, out=None):
        if out is None:
            out = np.empty(self.shape, self.dtype)
        b = self.batch
        b._check(b.lib.soccer_memcpy_d2h(b.h, out.ctypes.data, self.ptr, self.nbytes))
        return out

    def fill(self, value):
        b = self.batch
        b._check(b.lib.soccer_memset(b.h, self.ptr, int(value), self.nbytes))
        return self

    def row(self, k):
        """Device pointer of row k of a 2-D buffer."""
        return self.ptr + int(k) * self.shape[-1] * self.dtype.itemsize

    def free(self):
        if self.ptr and self.batch.h:
            self.batch.lib.soccer_free(self.batch.h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _ptr(x):
    """Device pointer of a DeviceArray / torch tensor / int / None."""
    if x is None:
        return None
    if isinstance(x, DeviceArray):
        return x.ptr
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):          # torch tensor on the handle's device
        return x.data_ptr()
    raise TypeError("expected a DeviceArray, a device tensor or an integer address, got %r" % type(x))


def minimax_q_config(nS, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, opponent="uniform"):
    """Checks the parameters of a minimax-Q learner (AssertionError, before any library call) and returns
    (soccer_minimax_q_config, the array it points into or None)."""
    g, a, d, e, q0 = float(discount_factor), float(alpha), float(decay), float(explor), float(q_init)
    assert 0.0 <= g < 1.0, "discount_factor must be in [0, 1)"
    assert 0.0 <= a <= 1.0, "alpha must be in [0, 1]"
    assert 0.0 < d <= 1.0, "decay must be in (0, 1]"
    assert 0.0 <= e <= 1.0, "explor must be in [0, 1]"
    assert -1.0 <= q0 <= 1.0, "q_init must be in [-1, 1]"
    pol = None
    if isinstance(opponent, str):
        assert opponent in ("uniform", "self"), "opponent must be 'uniform', 'self' or an [nS, 5] mixed policy"
        kind = _lib.MQ_UNIFORM if opponent == "uniform" else _lib.MQ_SELF
    else:
        pol = np.ascontiguousarray(opponent, np.float64)
        assert pol.shape == (int(nS), 5) and (pol >= 0).all() and np.allclose(pol.sum(1), 1.0), \
            "a fixed opponent must be [n_states, 5] rows summing to 1"
        kind = _lib.MQ_FIXED
    return _lib.MinimaxQConfig(g, a, d, e, q0, kind, 0, None if pol is None else pol.ctypes.data), pol


def _learner_update(b, call, q, obs, act_a, act_b, reward, terminated, next_obs):
    """a learner's update(): numpy arrays are copied to the device first and freed after the call"""
    args = (obs, act_a, act_b, reward, terminated, next_obs)
    dts = (np.uint16, np.int8, np.int8, np.int8, np.uint8, np.uint16)
    tmp = []
    if all(isinstance(x, (np.ndarray, list, tuple)) for x in args):
        host = [np.ascontiguousarray(x, dt).reshape(-1) for x, dt in zip(args, dts)]
        n = host[0].size
        assert all(x.size == n for x in host), "the six transition arrays must have one length"
        assert n <= _lib.MQ_MAX_LANES, "at most 2**22 transitions per update"
        if n:
            tmp = [DeviceArray(b, n, dt).upload(x) for x, dt in zip(host, dts)]
        ptrs = [a.ptr for a in tmp] if n else [None] * 6
    else:
        def length(x):
            return int(np.prod(x.shape)) if hasattr(x, "shape") else None
        n = length(obs)
        assert n is not None and all(length(x) == n for x in args), "the six transition arrays must have one length"
        ptrs = [_ptr(x) for x in args]
    try:
        b._check(call(b.h, q, n, *ptrs))
    finally:
        if tmp:
            b.sync()
            for a in tmp:
                a.free()


class _Learner:
    """What the six wrappers of a C learner share: they keep the batch and the learner, run() and close().  _C is the prefix
    of the kind's C entry points: _C + "_create", "_run", "_destroy"."""
    _C = None

    def _create(self, batch, cfg, *league):
        """the C learner of a config, whose arrays the caller keeps alive until this returns (create copies what it needs);
        league: what soccer_q_population_create_league takes between the config and the result"""
        self.batch, self.q = batch, None
        q = C.c_void_p()
        create = getattr(batch.lib, self._C + ("_create_league" if league else "_create"))
        batch._check(create(batch.h, C.byref(cfg), *league, C.byref(q)))
        self.q, self.nS = q, batch.nS
        batch._learners.add(self)

    def run(self, n_steps):
        """n_steps learner steps (every lane acts, the environment steps, the kind's tables and policies are updated; a
        population: every member's, from its lane), enqueued."""
        b = self.batch
        b._check(getattr(b.lib, self._C + "_run")(b.h, self.q, int(n_steps)))
        return self

    def close(self):
        if self.q and self.batch.h:
            getattr(self.batch.lib, self._C + "_destroy")(self.batch.h, self.q)
        self.q = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Population(_Learner):
    """What the three populations share: a member per lane with its own discount, ranges of members, update()."""

    def _create(self, batch, cfg, per_member, *league):
        """per_member: the config function's arrays of per-member hyperparameters (None: the scalar for every member)"""
        super()._create(batch, cfg, *league)
        self.n = batch.n
        gam = per_member["discount_factor"]
        self.discount_factor = np.full(batch.n, cfg.discount_factor) if gam is None else gam.copy()

    def update(self, obs, act_a, act_b, reward, terminated, next_obs):
        """One step's update on n transitions, transition i for member i (reward is player A's): DeviceArrays (or device
        tensors) of n elements, or numpy arrays, which are copied to the device first."""
        n = self.n

        def call(h, q, count, *ptrs):
            assert count == n, "a population's update takes one transition per member (%d)" % n
            return getattr(self.batch.lib, self._C + "_update")(h, q, *ptrs)
        _learner_update(self.batch, call, self.q, obs, act_a, act_b, reward, terminated, next_obs)
        return self

    def _range(self, first, count):
        first = int(first)
        count = self.n - first if count is None else int(count)
        assert 0 <= first <= self.n and 0 <= count <= self.n - first, "members %d .. %d + %d are outside the population of %d" % (first, first, count, self.n)
        return first, count

    def cross_play(self, theta=1e-10, first=0, count=None, discount_factor=None):
        """What each member's player A scores against each member's player B: (payoff[count, count], iterations) of
        SoccerBatch.cross_play on pi_a and pi_b (Q-learners: the one-hot greedy policies) of members first ..
        first + count - 1 (at most 1024).  discount_factor None: the range's common discount, ValueError if the members differ."""
        return _population_cross_play(self, self._policies, "pi_a", "pi_b", theta, first, count, discount_factor)

    def meta_game(self, theta=1e-10, first=0, count=None, discount_factor=None, max_pivots=None):
        """cross_play with the same arguments, then its meta-game solved (planners.meta_game): the members' mixture a rational
        opponent cannot beat, x, y, value, lo, hi, status, and gain = lo - the best single member's row_min."""
        return _meta_of_cross_play(self.batch, *self.cross_play(theta, first, count, discount_factor), max_pivots)

    def match_outcomes(self, theta=1e-10, first=0, count=None, continue_prob=None):
        """How often each member's player A beats each member's player B, how often they draw and how long they play:
        SoccerBatch.match_outcomes' dict on cross_play's policies of members first .. first + count - 1 (at most 1024).
        continue_prob None: the range's common discount, ValueError if the members differ."""
        return _population_match_outcomes(self, self._policies, "pi_a", "pi_b", theta, first, count, continue_prob)

    def occupancy(self, theta=1e-10, first=0, count=None, continue_prob=None, features=None, values=False):
        """Where each member's player A and each member's player B play their game: SoccerBatch.occupancy's dict on cross_play's
        policies of members first .. first + count - 1 (at most 1024).  continue_prob None: the range's common discount,
        ValueError if the members differ."""
        return _population_occupancy(self, self._policies, "pi_a", "pi_b", theta, first, count, continue_prob, features, values)


class MinimaxQLearner(_Learner):
    """A minimax-Q learner (Littman 1994) on a two-player auto-reset SoccerBatch: one shared Q[nS, 5, 5] on the device,
    the batch's lanes as actors (include/soccer_hip.h, "learners").  run() enqueues and returns; the properties
    synchronise and copy."""
    _C = "soccer_minimax_q"

    def __init__(self, batch, discount_factor, **params):
        cfg, keep = minimax_q_config(batch.nS, discount_factor, **params)
        self._create(batch, cfg)
        del keep                                   # (create has copied the opponent's thresholds)
        self.discount_factor = float(discount_factor)

    def update(self, obs, act_a, act_b, reward, terminated, next_obs):
        """One learner step's reduce / update / re-solve on a batch of transitions: DeviceArrays (or device tensors) of one
        length, or numpy arrays, which are copied to the device first."""
        _learner_update(self.batch, self.batch.lib.soccer_minimax_q_update, self.q, obs, act_a, act_b, reward, terminated, next_obs)
        return self

    def read(self):
        """dict: Q[nS, 5, 5], V[nS], pi_a / pi_b [nS, 5], visits[nS, 25], alpha, steps (synchronises)."""
        nS, b = self.nS, self.batch
        out = {"Q": np.zeros((nS, 5, 5)), "V": np.zeros(nS), "pi_a": np.zeros((nS, 5)), "pi_b": np.zeros((nS, 5)),
               "visits": np.zeros((nS, 25), np.uint64)}
        al, st = C.c_double(), C.c_uint64()
        b._check(b.lib.soccer_minimax_q_read(b.h, self.q, *[out[k].ctypes.data for k in ("Q", "V", "pi_a", "pi_b", "visits")],
                                             C.byref(al), C.byref(st)))
        out["alpha"], out["steps"] = float(al.value), int(st.value)
        return out

    def _one(self, key, shape, dtype=np.float64):
        b = self.batch
        a = np.zeros(shape, dtype)
        ptrs = [a.ctypes.data if k == key else None for k in ("Q", "V", "pi_a", "pi_b", "visits")]
        b._check(b.lib.soccer_minimax_q_read(b.h, self.q, *ptrs, None, None))
        return a

    Q = property(lambda self: self._one("Q", (self.nS, 5, 5)))
    V = property(lambda self: self._one("V", self.nS))
    pi_a = property(lambda self: self._one("pi_a", (self.nS, 5)))
    pi_b = property(lambda self: self._one("pi_b", (self.nS, 5)))
    visits = property(lambda self: self._one("visits", (self.nS, 25), np.uint64))

    @property
    def alpha(self):
        b, al = self.batch, C.c_double()
        b._check(b.lib.soccer_minimax_q_read(b.h, self.q, None, None, None, None, None, C.byref(al), None))
        return float(al.value)

    @property
    def steps(self):
        b, st = self.batch, C.c_uint64()
        b._check(b.lib.soccer_minimax_q_read(b.h, self.q, None, None, None, None, None, None, C.byref(st)))
        return int(st.value)

    def exploitability(self, theta=1e-10):
        """How badly the best possible opponent beats the strategies the learner holds now, at its discount:
        planners.exploitability of (pi_a, pi_b).  Synchronises and copies; run() does not."""
        from . import planners
        r = self.read()
        return planners.exploitability(self.batch, r["pi_a"], r["pi_b"], theta, self.discount_factor)

    def load(self, Q, visits=None, alpha=None, steps=None):
        """Resume from a checkpoint: Q[nS, 5, 5] in, V and the strategies re-solved on the device.  With `visits` (and the
        `alpha` / `steps` of read()) a fresh learner continues bit for bit; without, every state is solved."""
        b = self.batch
        Q = np.ascontiguousarray(Q, np.float64)
        assert Q.shape == (self.nS, 5, 5), "Q must be [n_states, 5, 5]"
        assert (np.abs(Q[1:]) <= 1.0).all(), "Q must lie in [-1, 1]"
        v = None
        if visits is not None:
            v = np.ascontiguousarray(visits, np.uint64)
            assert v.shape == (self.nS, 25), "visits must be [n_states, 25]"
        assert alpha is None or 0.0 <= float(alpha) <= 1.0, "alpha must be in [0, 1]"
        al = None if alpha is None else C.byref(C.c_double(float(alpha)))
        st = None if steps is None else C.byref(C.c_uint64(int(steps)))
        b._check(b.lib.soccer_minimax_q_load(b.h, self.q, Q.ctypes.data, None if v is None else v.ctypes.data, al, st))
        return self


def q_learning_config(nS, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, act_a="greedy", act_b="greedy"):
    """Checks the parameters of the independent Q-learners (AssertionError, before any library call) and returns
    (soccer_q_learner_config, the arrays it points into)."""
    g, a, d, e, q0 = float(discount_factor), float(alpha), float(decay), float(explor), float(q_init)
    assert 0.0 <= g < 1.0, "discount_factor must be in [0, 1)"
    assert 0.0 <= a <= 1.0, "alpha must be in [0, 1]"
    assert 0.0 < d <= 1.0, "decay must be in (0, 1]"
    assert 0.0 <= e <= 1.0, "explor must be in [0, 1]"
    assert -1.0 <= q0 <= 1.0, "q_init must be in [-1, 1]"
    kinds, pols = [], []
    for name, act in (("act_a", act_a), ("act_b", act_b)):
        pol = None
        if isinstance(act, str):
            assert act in ("greedy", "uniform"), "%s must be 'greedy', 'uniform' or an [nS, 5] mixed policy" % name
            kinds.append(_lib.QL_GREEDY if act == "greedy" else _lib.QL_UNIFORM)
        else:
            pol = np.ascontiguousarray(act, np.float64)
            assert pol.shape == (int(nS), 5) and (pol >= 0).all() and np.allclose(pol.sum(1), 1.0), \
                "a fixed %s must be [n_states, 5] rows summing to 1" % name
            kinds.append(_lib.QL_FIXED)
        pols.append(pol)
    return _lib.QLearnerConfig(g, a, d, e, q0, kinds[0], kinds[1], *[None if x is None else x.ctypes.data for x in pols]), pols


class QLearner(_Learner):
    """Independent Q-learners for both players (Littman 1994's baseline and challenger) on a two-player auto-reset
    SoccerBatch: Q_a[nS, 5] and Q_b[nS, 5] (player B's in its own reward) on the device, the batch's lanes as actors
    (include/soccer_hip.h, "learners, independent Q").  run() enqueues and returns; read() and the properties synchronise
    and copy."""
    _C = "soccer_q_learner"

    def __init__(self, batch, discount_factor, **params):
        cfg, keep = q_learning_config(batch.nS, discount_factor, **params)
        self._create(batch, cfg)
        del keep                                   # (create has copied the fixed policies' thresholds)
        self.discount_factor = float(discount_factor)

    def update(self, obs, act_a, act_b, reward, terminated, next_obs):
        """One learner step's reduce / update on a batch of transitions (reward is player A's): DeviceArrays (or device
        tensors) of one length, or numpy arrays, which are copied to the device first."""
        _learner_update(self.batch, self.batch.lib.soccer_q_learner_update, self.q, obs, act_a, act_b, reward, terminated, next_obs)
        return self

    def read(self):
        """dict: Q_a / Q_b [nS, 5], V_a / V_b [nS] (the row maxima), pi_a / pi_b [nS, 5] (one-hot of the first greedy action:
        they plug into rollout(mixed_policies=...) and planners.exploitability as they are; row 0, the terminal observation,
        is whatever argmax of zeros gives and is never read), visits[nS, 25], alpha, steps.  Synchronises."""
        nS, b = self.nS, self.batch
        out = {"Q_a": np.zeros((nS, 5)), "Q_b": np.zeros((nS, 5)), "visits": np.zeros((nS, 25), np.uint64)}
        al, st = C.c_double(), C.c_uint64()
        b._check(b.lib.soccer_q_learner_read(b.h, self.q, *[out[k].ctypes.data for k in ("Q_a", "Q_b", "visits")],
                                             C.byref(al), C.byref(st)))
        for p in "ab":
            out["V_" + p] = out["Q_" + p].max(1)
            out["pi_" + p] = np.eye(5)[out["Q_" + p].argmax(1)]
        out["alpha"], out["steps"] = float(al.value), int(st.value)
        return out

    @property
    def alpha(self):
        b, al = self.batch, C.c_double()
        b._check(b.lib.soccer_q_learner_read(b.h, self.q, None, None, None, C.byref(al), None))
        return float(al.value)

    @property
    def steps(self):
        b, st = self.batch, C.c_uint64()
        b._check(b.lib.soccer_q_learner_read(b.h, self.q, None, None, None, None, C.byref(st)))
        return int(st.value)

    def exploitability(self, theta=1e-10):
        """How badly the best possible opponent beats the greedy pair the learners hold now, at their discount:
        planners.exploitability of (pi_a, pi_b).  Synchronises and copies; run() does not."""
        from . import planners
        r = self.read()
        return planners.exploitability(self.batch, r["pi_a"], r["pi_b"], theta, self.discount_factor)

    def load(self, Q_a, Q_b, visits=None, alpha=None, steps=None):
        """Resume from a checkpoint: Q_a / Q_b [nS, 5] in; everything derived from them is recomputed on the device.  With
        the `visits`, `alpha` and `steps` of read() a fresh learner continues bit for bit; without `visits` the counts are
        zeroed."""
        b = self.batch
        Q = [np.ascontiguousarray(x, np.float64) for x in (Q_a, Q_b)]
        for x in Q:
            assert x.shape == (self.nS, 5), "Q_a / Q_b must be [n_states, 5]"
            assert (np.abs(x[1:]) <= 1.0).all(), "Q must lie in [-1, 1]"
        v = None
        if visits is not None:
            v = np.ascontiguousarray(visits, np.uint64)
            assert v.shape == (self.nS, 25), "visits must be [n_states, 25]"
        assert alpha is None or 0.0 <= float(alpha) <= 1.0, "alpha must be in [0, 1]"
        al = None if alpha is None else C.byref(C.c_double(float(alpha)))
        st = None if steps is None else C.byref(C.c_uint64(int(steps)))
        b._check(b.lib.soccer_q_learner_load(b.h, self.q, Q[0].ctypes.data, Q[1].ctypes.data, None if v is None else v.ctypes.data, al, st))
        return self


def league_config(nS, act_a, act_b, league_policies, league_weights):
    """Checks a league (AssertionError, before any library call): exactly one of act_a / act_b is "league", and then
    league_policies is [K, nS, 5] rows summing to 1 and league_weights [K] values >= 0 summing to 1, K in 1 .. 1024.
    Returns None without a league, else (player, K, policies, weights) with the arrays contiguous float64."""
    sides = [isinstance(a, str) and a == "league" for a in (act_a, act_b)]
    if not any(sides):
        assert league_policies is None and league_weights is None, "league_policies / league_weights go with act_a or act_b = 'league'"
        return None
    assert not all(sides), "exactly one player may be a league, not both"
    assert league_policies is not None and league_weights is not None, "a league needs league_policies [K, n_states, 5] and league_weights [K]"
    pol = np.ascontiguousarray(league_policies, np.float64)
    w = np.ascontiguousarray(league_weights, np.float64)
    assert pol.ndim == 3 and pol.shape[1:] == (int(nS), 5), "league_policies must be [K, n_states, 5]"
    K = pol.shape[0]
    assert 1 <= K <= _lib.LEAGUE_MAX_POLICIES, "a league holds 1 .. %d policies, not %d" % (_lib.LEAGUE_MAX_POLICIES, K)
    assert w.shape == (K,), "league_weights must hold one weight per league policy (%d)" % K
    bad = np.flatnonzero(~(np.isfinite(w) & (w >= 0)))
    assert bad.size == 0, "league_weights[%d] is negative or not a finite number" % (bad[0] if bad.size else -1)
    assert np.allclose(w.sum(), 1.0), "league_weights does not sum to 1"
    rows = (pol >= 0).all(2) & np.isclose(pol.sum(2), 1.0)
    bad = np.argwhere(~rows)
    assert bad.size == 0, "league_policies[%d][%d] is not a row >= 0 summing to 1" % (tuple(bad[0]) if bad.size else (-1, -1))
    return sides.index(True), K, pol, w


def q_population_config(n, nS, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, act_a="greedy", act_b="greedy",
                        league=None):
    """Checks the parameters of a population of Q-learners (AssertionError, before any library call) and returns
    (soccer_q_population_config, the arrays it points into).  discount_factor, alpha, decay and explor are scalars for every
    member or arrays of n, one value per member.  league: league_config's tuple, or None; its player is SOCCER_QL_FIXED
    with a NULL policy in the config."""
    if league is not None:                      # (the other checks see a placeholder for the league's player)
        act_a, act_b = ("uniform", act_b) if league[0] == 0 else (act_a, "uniform")
    ranges = (("discount_factor", discount_factor, lambda x: (0.0 <= x) & (x < 1.0), "[0, 1)"),
              ("alpha", alpha, lambda x: (0.0 <= x) & (x <= 1.0), "[0, 1]"),
              ("decay", decay, lambda x: (0.0 < x) & (x <= 1.0), "(0, 1]"),
              ("explor", explor, lambda x: (0.0 <= x) & (x <= 1.0), "[0, 1]"))
    scalars, arrays = {}, {}
    for name, value, ok, rng in ranges:
        if np.ndim(value) == 0:
            scalars[name], arrays[name] = float(value), None
            assert ok(scalars[name]), "%s must be in %s" % (name, rng)
        else:
            a = np.ascontiguousarray(value, np.float64)
            assert a.shape == (int(n),), "a per-member %s must have one value per lane (%d)" % (name, n)
            assert ok(a).all(), "every per-member %s must be in %s" % (name, rng)
            scalars[name], arrays[name] = float(a[0]), a
    # (the scalar checks of q_learning_config hold for the kinds, the fixed policies and q_init)
    base, pols = q_learning_config(nS, scalars["discount_factor"], scalars["alpha"], scalars["decay"], scalars["explor"], q_init, act_a, act_b)
    cfg = _lib.QPopulationConfig(base.discount_factor, base.alpha, base.decay, base.explor, base.q_init, base.act_a, base.act_b,
                                 base.policy_a, base.policy_b,
                                 *[None if arrays[k] is None else arrays[k].ctypes.data for k in ("alpha", "decay", "explor", "discount_factor")])
    if league is not None:
        setattr(cfg, "act_b" if league[0] else "act_a", _lib.QL_FIXED)
    return cfg, (pols, arrays)


def _population_cross_play(pop, read, key_a, key_b, theta, first, count, discount_factor):
    """Members first .. first + count - 1 of a population against one another (SoccerBatch.cross_play): player A's policies
    read(first, count)[key_a] meet the same members' player-B policies [key_b], read in chunks of at most 256 members."""
    pa, pb, discount_factor = _population_sides(pop, read, key_a, key_b, first, count, discount_factor, "cross_play", "discount_factor")
    return pop.batch.cross_play(pa, pb, theta, discount_factor)


def _population_match_outcomes(pop, read, key_a, key_b, theta, first, count, continue_prob):
    """_population_cross_play's members and policies through SoccerBatch.match_outcomes; continue_prob None: the range's
    common discount"""
    pa, pb, continue_prob = _population_sides(pop, read, key_a, key_b, first, count, continue_prob, "match_outcomes", "continue_prob")
    return pop.batch.match_outcomes(pa, pb, theta, continue_prob)


def _population_occupancy(pop, read, key_a, key_b, theta, first, count, continue_prob, features, values):
    """_population_cross_play's members and policies through SoccerBatch.occupancy; continue_prob None: the range's common
    discount"""
    pa, pb, continue_prob = _population_sides(pop, read, key_a, key_b, first, count, continue_prob, "occupancy", "continue_prob")
    return pop.batch.occupancy(pa, pb, theta, continue_prob, features=features, values=values)


def _population_sides(pop, read, key_a, key_b, first, count, discount, what, name):
    """(pi_a[count, nS, 5], pi_b[count, nS, 5], the discount) of members first .. first + count - 1; discount None: the one
    they share, ValueError if they differ"""
    first, count = pop._range(first, count)
    assert 1 <= count <= _lib.CROSS_MAX_POLICIES, "%s takes 1 .. %d members, not %d" % (what, _lib.CROSS_MAX_POLICIES, count)
    gam = pop.discount_factor[first:first + count]
    if discount is None:
        other = np.flatnonzero(gam != gam[0])
        if other.size:
            raise ValueError("members %d and %d have different discounts (%r and %r): pass %s" % (
                first, first + other[0], float(gam[0]), float(gam[other[0]]), name))
        discount = float(gam[0])
    pa = np.zeros((count, pop.nS, 5)); pb = np.zeros((count, pop.nS, 5))
    for c0 in range(0, count, _lib.BR_MAX_POLICIES):
        c = min(_lib.BR_MAX_POLICIES, count - c0)
        r = read(first + c0, c)
        pa[c0:c0 + c] = r[key_a]; pb[c0:c0 + c] = r[key_b]
    return pa, pb, float(discount)


def meta_lds_bytes(n_a, n_b):
    """The LDS a workgroup of the meta-game's LDS kernel takes for an n_a x n_b game (include/soccer_hip.h, "the meta-game"):
    path=1 of solve_meta_game needs this to be at most the device's limit, 163 840 bytes on gfx950."""
    stride = (n_a + n_b + 2) | 1
    return 128 + 8 * ((n_a + 2) * stride + n_a + 1) + 4 * n_a


def _meta_of_cross_play(batch, payoff, iterations, max_pivots):
    """cross-play's dict (planners.cross_play) plus the solved meta-game and what mixing buys player A"""
    row_min, col_max = payoff.min(1), payoff.max(0)
    out = {"payoff": payoff, "iterations": iterations, "row_min": row_min, "col_max": col_max,
           "bounds": (float(row_min.max()), float(col_max.min()))}
    m = batch.solve_meta_game(payoff, max_pivots=max_pivots)
    out.update({k: m[k] for k in ("x", "y", "value", "lo", "hi", "status")})
    out["gain"] = out["lo"] - out["bounds"][0]
    return out


class QPopulation(_Population):
    """A population of independent Q-learners on a two-player auto-reset SoccerBatch, a learner per lane: member i has its own
    Q_a[nS, 5], Q_b[nS, 5] and alpha and learns from lane i alone (include/soccer_hip.h, "learners, a population of
    independent Q-learners").  run() enqueues and returns; read() and the properties synchronise and copy.  Whole populations
    run to gigabytes, so read(), load() and exploitability() take a range of members."""
    _C = "soccer_q_population"

    def __init__(self, batch, discount_factor, league_policies=None, league_weights=None, **params):
        lg = league_config(batch.nS, params.get("act_a", "greedy"), params.get("act_b", "greedy"), league_policies, league_weights)
        cfg, keep = q_population_config(batch.n, batch.nS, discount_factor, league=lg, **params)
        self.league, self.n_policies = (None, 0) if lg is None else lg[:2]      # the league's player (0 = A, 1 = B) and its K
        self._create(batch, cfg, keep[1], *(() if lg is None else (lg[0], lg[1], lg[2].ctypes.data, lg[3].ctypes.data)))
        del keep                                   # (create has copied the parameters and the fixed policies' thresholds)

    def _policies(self, first, count):
        return self.read(first, count)

    def read(self, first=0, count=None):
        """dict for members first .. first + count - 1 (count None: to the end): Q_a / Q_b [count, nS, 5], V_a / V_b
        [count, nS] (the row maxima), pi_a / pi_b [count, nS, 5] (one-hot of the first greedy action), alpha[count], steps.
        Synchronises."""
        first, count = self._range(first, count)
        nS, b = self.nS, self.batch
        out = {"Q_a": np.zeros((count, nS, 5)), "Q_b": np.zeros((count, nS, 5)), "alpha": np.zeros(count)}
        st = C.c_uint64()
        b._check(b.lib.soccer_q_population_read(b.h, self.q, first, count, *[out[k].ctypes.data for k in ("Q_a", "Q_b", "alpha")], C.byref(st)))
        for p in "ab":
            out["V_" + p] = out["Q_" + p].max(2)
            out["pi_" + p] = np.eye(5)[out["Q_" + p].argmax(2)]
        out["steps"] = int(st.value)
        return out

    @property
    def alpha(self):
        """every member's learning rate, [n]"""
        b, al = self.batch, np.zeros(self.n)
        b._check(b.lib.soccer_q_population_read(b.h, self.q, 0, self.n, None, None, al.ctypes.data, None))
        return al

    @property
    def steps(self):
        b, st = self.batch, C.c_uint64()
        b._check(b.lib.soccer_q_population_read(b.h, self.q, 0, 0, None, None, None, C.byref(st)))
        return int(st.value)

    def exploitability(self, theta=1e-10, first=0, count=None):
        """How badly the best possible opponent beats the greedy pair of each member of a range, at that member's discount:
        the one-hot greedy policies go through SoccerBatch.best_response in batches of at most 256 members with one
        discount.  Returns {"v_a", "v_b", "gap"}, arrays of [count, nS] (planners.exploitability's per member)."""
        first, count = self._range(first, count)
        b = self.batch
        out = {k: np.zeros((count, self.nS)) for k in ("v_a", "v_b", "gap")}
        for c0 in range(0, count, _lib.BR_MAX_POLICIES):
            c = min(_lib.BR_MAX_POLICIES, count - c0)
            r = self.read(first + c0, c)
            gam = self.discount_factor[first + c0:first + c0 + c]
            for g in np.unique(gam):                # (one solve per discount in the chunk: a batch shares its discount)
                idx = np.flatnonzero(gam == g)
                out["v_a"][c0 + idx] = b.best_response(r["pi_a"][idx], 0, theta, float(g))[1]
                out["v_b"][c0 + idx] = b.best_response(r["pi_b"][idx], 1, theta, float(g))[1]
        out["gap"] = out["v_b"] - out["v_a"]
        return out

    def picks(self, first=0, count=None):
        """A league population's picks, int32[count]: the league policy each member's lane follows until its episode ends,
        -1 where the next step draws one.  Synchronises.  AssertionError on a population without a league."""
        first, count = self._range(first, count)
        b, out = self.batch, np.zeros(count, np.int32)
        b._check(b.lib.soccer_q_population_league_read(b.h, self.q, first, count, out.ctypes.data))
        return out

    def load_picks(self, picks, first=0):
        """Resume the picks of members first .. first + len(picks) - 1: values in -1 .. K - 1, -1 forces a draw at the next
        step.  With read() + picks() a fresh population continues bit for bit via load() + load_picks(), mid-episode
        included.  A refused load changes nothing."""
        p = np.ascontiguousarray(picks, np.int32)
        assert p.ndim == 1, "picks must be a vector, one value per member"
        first, count = self._range(first, p.shape[0])
        b = self.batch
        b._check(b.lib.soccer_q_population_league_load(b.h, self.q, first, count, p.ctypes.data))
        return self

    def load(self, Q_a=None, Q_b=None, alpha=None, steps=None, first=0):
        """Resume members first .. first + count - 1 from a checkpoint: Q_a / Q_b [count, nS, 5] in [-1, 1] and alpha[count]
        (count is what the arrays hold; None = unchanged), steps for the population.  With what read() gave, a fresh
        population continues bit for bit.  A refused load changes nothing."""
        b = self.batch
        arrs = [None if x is None else np.ascontiguousarray(x, np.float64) for x in (Q_a, Q_b, alpha)]
        counts = {x.shape[0] for x in arrs if x is not None and x.ndim >= 1}
        assert len(counts) <= 1, "Q_a, Q_b and alpha must hold the same number of members"
        first, count = self._range(first, counts.pop() if counts else 0)
        for x in arrs[:2]:
            if x is not None:
                assert x.shape == (count, self.nS, 5), "Q_a / Q_b must be [count, n_states, 5]"
                assert (np.abs(x[:, 1:]) <= 1.0).all(), "Q must lie in [-1, 1]"
        if arrs[2] is not None:
            assert arrs[2].shape == (count,) and ((arrs[2] >= 0.0) & (arrs[2] <= 1.0)).all(), "alpha must be [count] values in [0, 1]"
        st = None if steps is None else C.byref(C.c_uint64(int(steps)))
        b._check(b.lib.soccer_q_population_load(b.h, self.q, first, count, *[None if x is None else x.ctypes.data for x in arrs], st))
        return self


def om_population_config(n, nS, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, act_a="greedy", act_b="greedy"):
    """Checks the parameters of a population of opponent-modelling Q-learners (AssertionError, before any library call) and
    returns (soccer_om_population_config, the arrays it points into): q_population_config's checks and layout, no league."""
    cfg, keep = q_population_config(n, nS, discount_factor, alpha, decay, explor, q_init, act_a, act_b)
    return _lib.OMPopulationConfig.from_buffer_copy(cfg), keep


def om_derive(Q, counts):
    """The derived values of an opponent-modelling Q-learner by the definition's expression (include/soccer_hip.h, "learners, a
    population of opponent-modelling Q-learners"), operation for operation, so they equal the device's: Q [..., 5, 5] (own
    action, other's action) and counts [..., 5] (uint64) -> (V [...], g [...])."""
    Q = np.asarray(Q, np.float64); counts = np.asarray(counts, np.uint64)
    n = counts.sum(-1, dtype=np.uint64)
    w = np.where((n > 0)[..., None], counts.astype(np.float64), 1.0)
    N = np.where(n > 0, n.astype(np.float64), 5.0)
    W = w[..., None, 0] * Q[..., 0]
    for k in range(1, 5):
        W = W + w[..., None, k] * Q[..., k]
    g = W.argmax(-1)                                # the first index that attains the maximum
    V = np.minimum(1.0, np.maximum(-1.0, np.take_along_axis(W, g[..., None], -1)[..., 0] / N))
    return V, g


def om_model(counts):
    """Counts [..., 5] of a player's actions as a mixed policy: the frequencies, 0.2 where nothing was seen; renormalised in
    float64 so that a row whose quotients sum an ulp off 1 is a policy row to the library."""
    c = np.asarray(counts, np.uint64).astype(np.float64)
    n = c.sum(-1, keepdims=True)
    m = np.where(n > 0, c / np.where(n > 0, n, 1.0), 0.2)
    return m / m.sum(-1, keepdims=True)


class OpponentModelPopulation(_Population):
    """A population of opponent-modelling Q-learners (joint-action learners; fictitious play in self-play) on a two-player
    auto-reset SoccerBatch, a learner per lane: member i has, per player, a joint-action table Q[nS, 5, 5] over (own action,
    the other's action) in that player's own reward and the counts C[nS, 5] of the other player's actions, and its alpha, and
    learns from lane i alone (include/soccer_hip.h, "learners, a population of opponent-modelling Q-learners").  A player
    answers the other's empirical frequencies greedily.  run() enqueues and returns; read() and the properties synchronise and
    copy.  read(), load() and exploitability() take a range of members (a member is 390 KB on 5x4)."""
    _C = "soccer_om_population"
    _WHICH = {"greedy": ("pi_a", "pi_b"), "model": ("model_a", "model_b")}

    def __init__(self, batch, discount_factor, **params):
        cfg, keep = om_population_config(batch.n, batch.nS, discount_factor, **params)
        self._create(batch, cfg, keep[1])
        del keep                                   # (create has copied the parameters and the fixed policies' thresholds)

    def _read(self, first, count, keys):
        """the library's arrays alone: any of Q_a, Q_b, C_a, C_b, alpha, steps"""
        nS, b = self.nS, self.batch
        shapes = {"Q_a": ((count, nS, 5, 5), np.float64), "Q_b": ((count, nS, 5, 5), np.float64), "C_a": ((count, nS, 5), np.uint64),
                  "C_b": ((count, nS, 5), np.uint64), "alpha": ((count,), np.float64)}
        out = {k: np.zeros(*shapes[k]) for k in keys if k != "steps"}
        st = C.c_uint64()
        b._check(b.lib.soccer_om_population_read(b.h, self.q, first, count, *[out[k].ctypes.data if k in out else None for k in shapes],
                                                 C.byref(st) if "steps" in keys else None))
        if "steps" in keys:
            out["steps"] = int(st.value)
        return out

    def read(self, first=0, count=None):
        """dict for members first .. first + count - 1 (count None: to the end): Q_a / Q_b [count, nS, 5, 5], C_a / C_b
        [count, nS, 5] (uint64), alpha[count], steps; and, computed here by the definition's expression, V_a / V_b [count, nS]
        and pi_a / pi_b [count, nS, 5] (one-hot of g); and model_a = C_b as frequencies (what B has seen A play; 0.2 where
        nothing was seen), model_b = C_a likewise.  Synchronises."""
        first, count = self._range(first, count)
        out = self._read(first, count, ("Q_a", "Q_b", "C_a", "C_b", "alpha", "steps"))
        for p, other in (("a", "b"), ("b", "a")):
            out["V_" + p], g = om_derive(out["Q_" + p], out["C_" + p])
            out["pi_" + p] = np.eye(5)[g]
            out["model_" + p] = om_model(out["C_" + other])
        return out

    alpha = property(lambda self: self._read(0, self.n, ("alpha",))["alpha"], doc="every member's learning rate, [n]")
    steps = property(lambda self: self._read(0, 0, ("steps",))["steps"])

    def exploitability(self, which="greedy", theta=1e-10, first=0, count=None):
        """How badly the best possible opponent beats the pair of greedy policies (which='greedy') or the pair of models
        (which='model': model_a, what B has seen A play, with model_b) of each member of a range, at that member's discount:
        through SoccerBatch.best_response in batches of at most 256 members with one discount.  Returns {"v_a", "v_b", "gap"},
        arrays of [count, nS] (planners.exploitability's per member)."""
        assert which in self._WHICH, "which must be 'greedy' or 'model'"
        ka, kb = self._WHICH[which]
        first, count = self._range(first, count)
        b = self.batch
        out = {k: np.zeros((count, self.nS)) for k in ("v_a", "v_b", "gap")}
        for c0 in range(0, count, _lib.BR_MAX_POLICIES):
            c = min(_lib.BR_MAX_POLICIES, count - c0)
            r = self.read(first + c0, c)
            gam = self.discount_factor[first + c0:first + c0 + c]
            for g in np.unique(gam):                # (one solve per discount in the chunk: a batch shares its discount)
                idx = np.flatnonzero(gam == g)
                out["v_a"][c0 + idx] = b.best_response(r[ka][idx], 0, theta, float(g))[1]
                out["v_b"][c0 + idx] = b.best_response(r[kb][idx], 1, theta, float(g))[1]
        out["gap"] = out["v_b"] - out["v_a"]
        return out

    def cross_play(self, which="greedy", theta=1e-10, first=0, count=None, discount_factor=None):
        """What each member's player A scores against each member's player B: (payoff[count, count], iterations) of
        SoccerBatch.cross_play on the greedy policies (which='greedy') or the models (which='model') of members first ..
        first + count - 1 (at most 1024).  discount_factor None: the range's common discount, ValueError if the members differ."""
        assert which in self._WHICH, "which must be 'greedy' or 'model'"
        return _population_cross_play(self, self.read, *self._WHICH[which], theta, first, count, discount_factor)

    def meta_game(self, which="greedy", theta=1e-10, first=0, count=None, discount_factor=None, max_pivots=None):
        """cross_play with the same arguments, then its meta-game solved (planners.meta_game): the members' mixture a rational
        opponent cannot beat, x, y, value, lo, hi, status, and gain = lo - the best single member's row_min."""
        return _meta_of_cross_play(self.batch, *self.cross_play(which, theta, first, count, discount_factor), max_pivots)

    def match_outcomes(self, which="greedy", theta=1e-10, first=0, count=None, continue_prob=None):
        """How often each member's player A beats each member's player B, how often they draw and how long they play:
        SoccerBatch.match_outcomes' dict on cross_play's policies (which) of members first .. first + count - 1 (at most 1024).
        continue_prob None: the range's common discount, ValueError if the members differ."""
        assert which in self._WHICH, "which must be 'greedy' or 'model'"
        return _population_match_outcomes(self, self.read, *self._WHICH[which], theta, first, count, continue_prob)

    def occupancy(self, which="greedy", theta=1e-10, first=0, count=None, continue_prob=None, features=None, values=False):
        """Where each member's player A and each member's player B play their game: SoccerBatch.occupancy's dict on cross_play's
        policies (which) of members first .. first + count - 1 (at most 1024).  continue_prob None: the range's common discount,
        ValueError if the members differ."""
        assert which in self._WHICH, "which must be 'greedy' or 'model'"
        return _population_occupancy(self, self.read, *self._WHICH[which], theta, first, count, continue_prob, features, values)

    def load(self, Q_a=None, Q_b=None, C_a=None, C_b=None, alpha=None, steps=None, first=0):
        """Resume members first .. first + count - 1 from a checkpoint (count is what the arrays hold; None = unchanged): Q_a /
        Q_b [count, nS, 5, 5] in [-1, 1], C_a / C_b [count, nS, 5] counts, alpha[count], steps for the population.  V and the
        greedy actions follow on the device.  With what read() gave, a fresh population continues bit for bit.  A refused
        load changes nothing."""
        b = self.batch
        arrs = [None if x is None else np.ascontiguousarray(x, dt) for x, dt in
                zip((Q_a, Q_b, C_a, C_b, alpha), (np.float64, np.float64, np.uint64, np.uint64, np.float64))]
        counts = {x.shape[0] for x in arrs if x is not None and x.ndim >= 1}
        assert len(counts) <= 1, "Q_a, Q_b, C_a, C_b and alpha must hold the same number of members"
        first, count = self._range(first, counts.pop() if counts else 0)
        for x in arrs[:2]:
            if x is not None:
                assert x.shape == (count, self.nS, 5, 5), "Q_a / Q_b must be [count, n_states, 5, 5]"
                assert (np.abs(x[:, 1:]) <= 1.0).all(), "Q must lie in [-1, 1]"
        for x in arrs[2:4]:
            assert x is None or x.shape == (count, self.nS, 5), "C_a / C_b must be [count, n_states, 5]"
        if arrs[4] is not None:
            assert arrs[4].shape == (count,) and ((arrs[4] >= 0.0) & (arrs[4] <= 1.0)).all(), "alpha must be [count] values in [0, 1]"
        st = None if steps is None else C.byref(C.c_uint64(int(steps)))
        b._check(b.lib.soccer_om_population_load(b.h, self.q, first, count, *[None if x is None else x.ctypes.data for x in arrs], st))
        return self


def wolf_phc_config(nS, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, delta_win=0.01, delta_lose=0.04,
                    delta_decay=1.0, act_a="learn", act_b="learn"):
    """Checks the parameters of the policy hill-climbers (AssertionError, before any library call) and returns
    (soccer_wolf_phc_config, the arrays it points into)."""
    g, a, d, e, q0 = float(discount_factor), float(alpha), float(decay), float(explor), float(q_init)
    dw, dl, dd = float(delta_win), float(delta_lose), float(delta_decay)
    assert 0.0 <= g < 1.0, "discount_factor must be in [0, 1)"
    assert 0.0 <= a <= 1.0, "alpha must be in [0, 1]"
    assert 0.0 < d <= 1.0, "decay must be in (0, 1]"
    assert 0.0 <= e <= 1.0, "explor must be in [0, 1]"
    assert -1.0 <= q0 <= 1.0, "q_init must be in [-1, 1]"
    assert 0.0 <= dw <= 1.0, "delta_win must be in [0, 1]"
    assert 0.0 <= dl <= 1.0, "delta_lose must be in [0, 1]"
    assert 0.0 < dd <= 1.0, "delta_decay must be in (0, 1]"
    kinds, pols = [], []
    for name, act in (("act_a", act_a), ("act_b", act_b)):
        pol = None
        if isinstance(act, str):
            assert act in ("learn", "uniform"), "%s must be 'learn', 'uniform' or an [nS, 5] mixed policy" % name
            kinds.append(_lib.PHC_LEARN if act == "learn" else _lib.PHC_UNIFORM)
        else:
            pol = np.ascontiguousarray(act, np.float64)
            assert pol.shape == (int(nS), 5) and (pol >= 0).all() and np.allclose(pol.sum(1), 1.0), \
                "a fixed %s must be [n_states, 5] rows summing to 1" % name
            kinds.append(_lib.PHC_FIXED)
        pols.append(pol)
    return _lib.WolfPHCConfig(g, a, d, e, q0, dw, dl, dd, kinds[0], kinds[1], *[None if x is None else x.ctypes.data for x in pols]), pols


class WolfPHCLearner(_Learner):
    """Policy hill-climbers for both players (PHC and WoLF-PHC, Bowling & Veloso 2002) on a two-player auto-reset
    SoccerBatch: the Q-learners' two tables plus a mixed policy pi_p[nS, 5] and its running average avg_p per player on
    the device, the batch's lanes as actors (include/soccer_hip.h, "learners, policy hill-climbing").  run() enqueues
    and returns; read() and the properties synchronise and copy."""
    _C = "soccer_wolf_phc"
    _ROWS = ("Q_a", "Q_b", "pi_a", "pi_b", "avg_a", "avg_b")

    def __init__(self, batch, discount_factor, **params):
        cfg, keep = wolf_phc_config(batch.nS, discount_factor, **params)
        self._create(batch, cfg)
        del keep                                   # (create has copied the fixed policies)
        self.discount_factor = float(discount_factor)

    def update(self, obs, act_a, act_b, reward, terminated, next_obs):
        """One learner step's reduce / update / policy step on a batch of transitions (reward is player A's): DeviceArrays
        (or device tensors) of one length, or numpy arrays, which are copied to the device first."""
        _learner_update(self.batch, self.batch.lib.soccer_wolf_phc_update, self.q, obs, act_a, act_b, reward, terminated, next_obs)
        return self

    def read(self):
        """dict: Q_a / Q_b, pi_a / pi_b, avg_a / avg_b [nS, 5], V_a / V_b [nS] (the row maxima, computed here), visits[nS, 25],
        updates[nS], alpha, dscale, steps.  The policies plug into rollout(mixed_policies=...) and planners.exploitability
        as they are.  Synchronises."""
        nS, b = self.nS, self.batch
        out = {k: np.zeros((nS, 5)) for k in self._ROWS}
        out["visits"] = np.zeros((nS, 25), np.uint64); out["updates"] = np.zeros(nS, np.uint64)
        al, ds, st = C.c_double(), C.c_double(), C.c_uint64()
        state = _lib.WolfPHCState(*[out[k].ctypes.data for k in self._ROWS + ("visits", "updates")],
                                  C.pointer(al), C.pointer(ds), C.pointer(st))
        b._check(b.lib.soccer_wolf_phc_read(b.h, self.q, C.byref(state)))
        for p in "ab":
            out["V_" + p] = out["Q_" + p].max(1)
        out["alpha"], out["dscale"], out["steps"] = float(al.value), float(ds.value), int(st.value)
        return out

    def _scalar(self, name, ctype):
        b, v = self.batch, ctype()
        state = _lib.WolfPHCState(**{name: C.pointer(v)})
        b._check(b.lib.soccer_wolf_phc_read(b.h, self.q, C.byref(state)))
        return v.value

    alpha = property(lambda self: float(self._scalar("alpha", C.c_double)))
    dscale = property(lambda self: float(self._scalar("dscale", C.c_double)))
    steps = property(lambda self: int(self._scalar("steps", C.c_uint64)))

    def exploitability(self, which="pi", theta=1e-10):
        """How badly the best possible opponent beats the pair of policies (which='pi') or of average policies
        (which='avg') the learners hold now, at their discount: planners.exploitability.  Synchronises and copies."""
        from . import planners
        assert which in ("pi", "avg"), "which must be 'pi' or 'avg'"
        r = self.read()
        return planners.exploitability(self.batch, r[which + "_a"], r[which + "_b"], theta, self.discount_factor)

    def load(self, Q_a, Q_b, pi_a=None, pi_b=None, avg_a=None, avg_b=None, visits=None, updates=None, alpha=None, dscale=None,
             steps=None):
        """Resume from a checkpoint: everything derived is recomputed on the device.  With all of read()'s arrays and
        scalars a fresh learner continues bit for bit.  A policy array that is None is left as it is (those of a player
        that does not learn are ignored); without `visits` / `updates` the counts are zeroed."""
        b = self.batch
        rows = {"Q_a": Q_a, "Q_b": Q_b, "pi_a": pi_a, "pi_b": pi_b, "avg_a": avg_a, "avg_b": avg_b}
        keep = {}
        for k, x in rows.items():
            if x is None:
                assert not k.startswith("Q"), "Q_a / Q_b are required"
                continue
            x = keep[k] = np.ascontiguousarray(x, np.float64)
            assert x.shape == (self.nS, 5), "%s must be [n_states, 5]" % k
            if k.startswith("Q"):
                assert (np.abs(x[1:]) <= 1.0).all(), "Q must lie in [-1, 1]"
        for k, x, shape in (("visits", visits, (self.nS, 25)), ("updates", updates, (self.nS,))):
            if x is not None:
                keep[k] = np.ascontiguousarray(x, np.uint64)
                assert keep[k].shape == shape, "%s must be %r" % (k, list(shape))
        assert alpha is None or 0.0 <= float(alpha) <= 1.0, "alpha must be in [0, 1]"
        assert dscale is None or 0.0 <= float(dscale) <= 1.0, "dscale must be in [0, 1]"
        state = _lib.WolfPHCState(**{k: x.ctypes.data for k, x in keep.items()})
        if alpha is not None:
            state.alpha = C.pointer(C.c_double(float(alpha)))
        if dscale is not None:
            state.dscale = C.pointer(C.c_double(float(dscale)))
        if steps is not None:
            state.steps = C.pointer(C.c_uint64(int(steps)))
        b._check(b.lib.soccer_wolf_phc_load(b.h, self.q, C.byref(state)))
        return self


_WOLF_HYPER = (("discount_factor", lambda x: (0.0 <= x) & (x < 1.0), "[0, 1)"), ("alpha", lambda x: (0.0 <= x) & (x <= 1.0), "[0, 1]"),
               ("decay", lambda x: (0.0 < x) & (x <= 1.0), "(0, 1]"), ("explor", lambda x: (0.0 <= x) & (x <= 1.0), "[0, 1]"),
               ("delta_win", lambda x: (0.0 <= x) & (x <= 1.0), "[0, 1]"), ("delta_lose", lambda x: (0.0 <= x) & (x <= 1.0), "[0, 1]"),
               ("delta_decay", lambda x: (0.0 < x) & (x <= 1.0), "(0, 1]"))


def wolf_population_config(n, nS, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, delta_win=0.01,
                           delta_lose=0.04, delta_decay=1.0, act_a="learn", act_b="learn"):
    """Checks the parameters of a population of policy hill-climbers (AssertionError, before any library call) and returns
    (soccer_wolf_population_config, the arrays it points into).  The seven hyperparameters are scalars for every member or
    arrays of n, one value per member; act_a / act_b: 'learn', 'uniform', one fixed [nS, 5] mixed policy for every member, or
    [n, nS, 5], a fixed policy per member."""
    given = dict(discount_factor=discount_factor, alpha=alpha, decay=decay, explor=explor, delta_win=delta_win, delta_lose=delta_lose,
                 delta_decay=delta_decay)
    scalars, arrays = {}, {}
    for name, ok, rng in _WOLF_HYPER:
        value = given[name]
        if np.ndim(value) == 0:
            scalars[name], arrays[name] = float(value), None
            assert ok(scalars[name]), "%s must be in %s" % (name, rng)
        else:
            a = np.ascontiguousarray(value, np.float64)
            assert a.shape == (int(n),), "a per-member %s must have one value per lane (%d)" % (name, n)
            assert ok(a).all(), "every per-member %s must be in %s" % (name, rng)
            scalars[name], arrays[name] = float(a[0]), a
    q0 = float(q_init)
    assert -1.0 <= q0 <= 1.0, "q_init must be in [-1, 1]"
    kinds, shared, each = [], [None, None], [None, None]
    for p, (name, act) in enumerate((("act_a", act_a), ("act_b", act_b))):
        if isinstance(act, str):
            assert act in ("learn", "uniform"), "%s must be 'learn', 'uniform', an [nS, 5] or an [n, nS, 5] mixed policy" % name
            kinds.append(_lib.PHC_LEARN if act == "learn" else _lib.PHC_UNIFORM)
            continue
        pol = np.ascontiguousarray(act, np.float64)
        assert pol.shape in ((int(nS), 5), (int(n), int(nS), 5)) and (pol >= 0).all() and np.allclose(pol.sum(-1), 1.0), \
            "a fixed %s must be [n_states, 5] or [n_lanes, n_states, 5] rows summing to 1" % name
        (shared if pol.ndim == 2 else each)[p] = pol
        kinds.append(_lib.PHC_FIXED)
    ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
    cfg = _lib.WolfPopulationConfig(scalars["discount_factor"], scalars["alpha"], scalars["decay"], scalars["explor"], q0,
                                    scalars["delta_win"], scalars["delta_lose"], scalars["delta_decay"], kinds[0], kinds[1],
                                    ptr(shared[0]), ptr(shared[1]), ptr(each[0]), ptr(each[1]),
                                    *[ptr(arrays[k]) for k in ("alpha", "decay", "explor", "discount_factor", "delta_win", "delta_lose", "delta_decay")])
    return cfg, ((shared, each), arrays)


class WolfPopulation(_Population):
    """A population of policy hill-climbers (PHC / WoLF-PHC) on a two-player auto-reset SoccerBatch, a learner per lane:
    member i has its own Q_a, Q_b, pi_a, pi_b, avg_a, avg_b [nS, 5], updates[nS], alpha and dscale and learns from lane i alone
    (include/soccer_hip.h, "learners, a population of policy hill-climbers").  A fixed player's policy is per member.  run()
    enqueues and returns; read() and the properties synchronise and copy.  read(), load() and exploitability() take a range
    of members."""
    _C = "soccer_wolf_population"
    _ROWS = ("Q_a", "Q_b", "pi_a", "pi_b", "avg_a", "avg_b")

    def __init__(self, batch, discount_factor, **params):
        cfg, keep = wolf_population_config(batch.n, batch.nS, discount_factor, **params)
        self._create(batch, cfg, keep[1])
        del keep                                   # (create has copied the parameters and the fixed policies)
        self.modes = (cfg.act_a, cfg.act_b)

    def _read(self, first, count, keys):
        nS, b = self.nS, self.batch
        shapes = {"updates": ((count, nS), np.uint64), "alpha": ((count,), np.float64), "dscale": ((count,), np.float64)}
        out = {k: np.zeros(*shapes.get(k, ((count, nS, 5), np.float64))) for k in keys if k != "steps"}
        st = C.c_uint64()
        state = _lib.WolfPopulationState(**{k: x.ctypes.data for k, x in out.items()})
        if "steps" in keys:
            state.steps = C.pointer(st)
        b._check(b.lib.soccer_wolf_population_read(b.h, self.q, first, count, C.byref(state)))
        if "steps" in keys:
            out["steps"] = int(st.value)
        return out

    def read(self, first=0, count=None):
        """dict for members first .. first + count - 1 (count None: to the end): Q_a / Q_b, pi_a / pi_b, avg_a / avg_b
        [count, nS, 5], V_a / V_b [count, nS] (the row maxima, computed here), updates[count, nS], alpha[count],
        dscale[count], steps.  Synchronises."""
        first, count = self._range(first, count)
        out = self._read(first, count, self._ROWS + ("updates", "alpha", "dscale", "steps"))
        for p in "ab":
            out["V_" + p] = out["Q_" + p].max(2)
        return out

    alpha = property(lambda self: self._read(0, self.n, ("alpha",))["alpha"], doc="every member's learning rate, [n]")
    dscale = property(lambda self: self._read(0, self.n, ("dscale",))["dscale"], doc="every member's factor on both deltas, [n]")
    steps = property(lambda self: self._read(0, 0, ("steps",))["steps"])

    def exploitability(self, which="pi", theta=1e-10, first=0, count=None):
        """How badly the best possible opponent beats the pair of policies (which='pi') or of average policies (which='avg')
        of each member of a range, at that member's discount: through SoccerBatch.best_response in batches of at most 256
        members with one discount.  Returns {"v_a", "v_b", "gap"}, arrays of [count, nS] (planners.exploitability's per
        member)."""
        assert which in ("pi", "avg"), "which must be 'pi' or 'avg'"
        first, count = self._range(first, count)
        b = self.batch
        out = {k: np.zeros((count, self.nS)) for k in ("v_a", "v_b", "gap")}
        for c0 in range(0, count, _lib.BR_MAX_POLICIES):
            c = min(_lib.BR_MAX_POLICIES, count - c0)
            r = self._read(first + c0, c, (which + "_a", which + "_b"))
            gam = self.discount_factor[first + c0:first + c0 + c]
            for g in np.unique(gam):                # (one solve per discount in the chunk: a batch shares its discount)
                idx = np.flatnonzero(gam == g)
                out["v_a"][c0 + idx] = b.best_response(r[which + "_a"][idx], 0, theta, float(g))[1]
                out["v_b"][c0 + idx] = b.best_response(r[which + "_b"][idx], 1, theta, float(g))[1]
        out["gap"] = out["v_b"] - out["v_a"]
        return out

    def cross_play(self, which="pi", theta=1e-10, first=0, count=None, discount_factor=None):
        """What each member's player A scores against each member's player B: (payoff[count, count], iterations) of
        SoccerBatch.cross_play on the policies (which='pi') or the average policies (which='avg') of members first ..
        first + count - 1 (at most 1024).  discount_factor None: the range's common discount, ValueError if the members differ."""
        assert which in ("pi", "avg"), "which must be 'pi' or 'avg'"
        return _population_cross_play(self, lambda f, c: self._read(f, c, (which + "_a", which + "_b")), which + "_a", which + "_b",
                                      theta, first, count, discount_factor)

    def meta_game(self, which="pi", theta=1e-10, first=0, count=None, discount_factor=None, max_pivots=None):
        """cross_play with the same arguments, then its meta-game solved (planners.meta_game): the members' mixture a rational
        opponent cannot beat, x, y, value, lo, hi, status, and gain = lo - the best single member's row_min."""
        return _meta_of_cross_play(self.batch, *self.cross_play(which, theta, first, count, discount_factor), max_pivots)

    def match_outcomes(self, which="pi", theta=1e-10, first=0, count=None, continue_prob=None):
        """How often each member's player A beats each member's player B, how often they draw and how long they play:
        SoccerBatch.match_outcomes' dict on cross_play's policies (which) of members first .. first + count - 1 (at most 1024).
        continue_prob None: the range's common discount, ValueError if the members differ."""
        assert which in ("pi", "avg"), "which must be 'pi' or 'avg'"
        return _population_match_outcomes(self, lambda f, c: self._read(f, c, (which + "_a", which + "_b")), which + "_a", which + "_b",
                                          theta, first, count, continue_prob)

    def occupancy(self, which="pi", theta=1e-10, first=0, count=None, continue_prob=None, features=None, values=False):
        """Where each member's player A and each member's player B play their game: SoccerBatch.occupancy's dict on cross_play's
        policies (which) of members first .. first + count - 1 (at most 1024).  continue_prob None: the range's common discount,
        ValueError if the members differ."""
        assert which in ("pi", "avg"), "which must be 'pi' or 'avg'"
        return _population_occupancy(self, lambda f, c: self._read(f, c, (which + "_a", which + "_b")), which + "_a", which + "_b",
                                     theta, first, count, continue_prob, features, values)

    def load(self, Q_a=None, Q_b=None, pi_a=None, pi_b=None, avg_a=None, avg_b=None, updates=None, alpha=None, dscale=None, steps=None,
             first=0):
        """Resume members first .. first + count - 1 from a checkpoint (count is what the arrays hold; None = unchanged): the
        six tables [count, nS, 5], updates[count, nS], alpha[count] and dscale[count], steps for the population.  With what
        read() gave, a fresh population continues bit for bit.  A refused load changes nothing."""
        b = self.batch
        keep = {k: np.ascontiguousarray(x, np.float64) for k, x in zip(self._ROWS + ("alpha", "dscale"), (Q_a, Q_b, pi_a, pi_b, avg_a, avg_b, alpha, dscale))
                if x is not None}
        if updates is not None:
            keep["updates"] = np.ascontiguousarray(updates, np.uint64)
        counts = {x.shape[0] for x in keep.values() if x.ndim >= 1}
        assert len(counts) <= 1 and all(x.ndim >= 1 for x in keep.values()), "the arrays must hold the same number of members"
        first, count = self._range(first, counts.pop() if counts else 0)
        for k, x in keep.items():
            if k in self._ROWS:
                assert x.shape == (count, self.nS, 5), "%s must be [count, n_states, 5]" % k
                if k.startswith("Q"):
                    assert (np.abs(x[:, 1:]) <= 1.0).all(), "Q must lie in [-1, 1]"
            elif k == "updates":
                assert x.shape == (count, self.nS), "updates must be [count, n_states]"
            else:
                assert x.shape == (count,) and ((x >= 0.0) & (x <= 1.0)).all(), "%s must be [count] values in [0, 1]" % k
        state = _lib.WolfPopulationState(**{k: x.ctypes.data for k, x in keep.items()})
        if steps is not None:
            state.steps = C.pointer(C.c_uint64(int(steps)))
        b._check(b.lib.soccer_wolf_population_load(b.h, self.q, first, count, C.byref(state)))
        return self

    def adopt(self, player, src, src_player, which="pi"):
        """Freeze: every member's fixed policy of `player` (0 = A, 1 = B) becomes the pi (which='pi') or avg (which='avg') of
        `src_player` of the same member of the population `src` on this batch, on the device, enqueued."""
        assert which in ("pi", "avg"), "which must be 'pi' or 'avg'"
        assert isinstance(src, WolfPopulation), "src must be a WolfPopulation"
        b = self.batch
        b._check(b.lib.soccer_wolf_population_adopt(b.h, self.q, int(player), src.q, int(src_player), 0 if which == "pi" else 1))
        return self

    def challengers(self, against, which="pi", **hyper):
        """A second population on the same batch for the challenger protocol: its player `against` (0 = A, 1 = B) is fixed,
        member by member, to this population's pi (or avg) of that player as it is now; its other player learns from scratch
        with the hyperparameters given (WolfPopulation's; default discount: this population's)."""
        assert against in (0, 1), "against must be 0 (player A is frozen) or 1 (player B)"
        assert "act_a" not in hyper and "act_b" not in hyper, "challengers() sets act_a / act_b"
        hyper.setdefault("discount_factor", self.discount_factor)
        acts = ["learn", "learn"]
        acts[against] = np.full((self.nS, 5), 0.2)          # a placeholder row table: adopt() overwrites every member's
        c = WolfPopulation(self.batch, hyper.pop("discount_factor"), act_a=acts[0], act_b=acts[1], **hyper)
        return c.adopt(against, self, against, which)


def minimax_q_population_config(n, nS, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, opponent="uniform"):
    """Checks the parameters of a population of minimax-Q learners (AssertionError, before any library call) and returns
    (soccer_minimax_q_population_config, the arrays it points into).  discount_factor, alpha, decay and explor are scalars
    for every member or arrays of n, one value per member; opponent: 'uniform', 'self', one fixed [nS, 5] mixed policy for
    every member, or [n, nS, 5], a fixed policy per member."""
    ranges = (("discount_factor", discount_factor, lambda x: (0.0 <= x) & (x < 1.0), "[0, 1)"),
              ("alpha", alpha, lambda x: (0.0 <= x) & (x <= 1.0), "[0, 1]"),
              ("decay", decay, lambda x: (0.0 < x) & (x <= 1.0), "(0, 1]"),
              ("explor", explor, lambda x: (0.0 <= x) & (x <= 1.0), "[0, 1]"))
    scalars, arrays = {}, {}
    for name, value, ok, rng in ranges:
        if np.ndim(value) == 0:
            scalars[name], arrays[name] = float(value), None
            assert ok(scalars[name]), "%s must be in %s" % (name, rng)
        else:
            a = np.ascontiguousarray(value, np.float64)
            assert a.shape == (int(n),), "a per-member %s must have one value per lane (%d)" % (name, n)
            assert ok(a).all(), "every per-member %s must be in %s" % (name, rng)
            scalars[name], arrays[name] = float(a[0]), a
    q0 = float(q_init)
    assert -1.0 <= q0 <= 1.0, "q_init must be in [-1, 1]"
    shared = each = None
    if isinstance(opponent, str):
        assert opponent in ("uniform", "self"), "opponent must be 'uniform', 'self', an [nS, 5] or an [n, nS, 5] mixed policy"
        kind = _lib.MQ_UNIFORM if opponent == "uniform" else _lib.MQ_SELF
    else:
        pol = np.ascontiguousarray(opponent, np.float64)
        assert pol.shape in ((int(nS), 5), (int(n), int(nS), 5)), "a fixed opponent must be [n_states, 5] or [n_lanes, n_states, 5] rows summing to 1"
        bad = np.argwhere(~((pol >= 0).all(-1) & np.isclose(pol.sum(-1), 1.0)))
        if bad.size:
            where = "state %d" % bad[0][0] if pol.ndim == 2 else "member %d, state %d" % tuple(bad[0])
            raise AssertionError("a fixed opponent must be [n_states, 5] or [n_lanes, n_states, 5] rows >= 0 summing to 1: %s is not" % where)
        if pol.ndim == 2:
            shared = pol
        else:
            each = pol
        kind = _lib.MQ_FIXED
    ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
    cfg = _lib.MinimaxQPopulationConfig(scalars["discount_factor"], scalars["alpha"], scalars["decay"], scalars["explor"], q0, kind, 0,
                                        ptr(shared), ptr(each), *[ptr(arrays[k]) for k in ("alpha", "decay", "explor", "discount_factor")])
    return cfg, ((shared, each), arrays)


class MinimaxQPopulation(_Population):
    """A population of minimax-Q learners (Littman 1994) on a two-player auto-reset SoccerBatch, a learner per lane: member i
    has its own Q[nS, 5, 5], V[nS], pi_a / pi_b [nS, 5] and alpha and learns from lane i alone (include/soccer_hip.h, "learners,
    a population of minimax-Q learners").  run() enqueues and returns; read() and the properties synchronise and copy.  Whole
    populations run to gigabytes, so read(), load() and exploitability() take a range of members."""
    _C = "soccer_minimax_q_population"
    _ROWS = ("Q", "V", "pi_a", "pi_b")

    def __init__(self, batch, discount_factor, **params):
        cfg, keep = minimax_q_population_config(batch.n, batch.nS, discount_factor, **params)
        self._create(batch, cfg, keep[1])
        del keep                                   # (create has copied the parameters and the fixed policies' thresholds)
        self.opponent = cfg.opponent

    def _policies(self, first, count):
        return self._read(first, count, ("pi_a", "pi_b"))

    def _read(self, first, count, keys):
        nS, b = self.nS, self.batch
        shapes = {"Q": (count, nS, 5, 5), "V": (count, nS), "pi_a": (count, nS, 5), "pi_b": (count, nS, 5), "alpha": (count,)}
        out = {k: np.zeros(shapes[k]) for k in keys if k != "steps"}
        st = C.c_uint64()
        b._check(b.lib.soccer_minimax_q_population_read(b.h, self.q, first, count,
                                                        *[out[k].ctypes.data if k in out else None for k in self._ROWS + ("alpha",)],
                                                        C.byref(st) if "steps" in keys else None))
        if "steps" in keys:
            out["steps"] = int(st.value)
        return out

    def read(self, first=0, count=None):
        """dict for members first .. first + count - 1 (count None: to the end): Q[count, nS, 5, 5], V[count, nS], pi_a / pi_b
        [count, nS, 5], alpha[count], steps.  Synchronises."""
        first, count = self._range(first, count)
        return self._read(first, count, self._ROWS + ("alpha", "steps"))

    alpha = property(lambda self: self._read(0, self.n, ("alpha",))["alpha"], doc="every member's learning rate, [n]")
    steps = property(lambda self: self._read(0, 0, ("steps",))["steps"])

    def exploitability(self, theta=1e-10, first=0, count=None):
        """How badly the best possible opponent beats the strategies pi_a and pi_b of each member of a range, at that member's
        discount: through SoccerBatch.best_response in batches of at most 256 members with one discount.  Returns
        {"v_a", "v_b", "gap"}, arrays of [count, nS] (planners.exploitability's per member)."""
        first, count = self._range(first, count)
        b = self.batch
        out = {k: np.zeros((count, self.nS)) for k in ("v_a", "v_b", "gap")}
        for c0 in range(0, count, _lib.BR_MAX_POLICIES):
            c = min(_lib.BR_MAX_POLICIES, count - c0)
            r = self._read(first + c0, c, ("pi_a", "pi_b"))
            gam = self.discount_factor[first + c0:first + c0 + c]
            for g in np.unique(gam):                # (one solve per discount in the chunk: a batch shares its discount)
                idx = np.flatnonzero(gam == g)
                out["v_a"][c0 + idx] = b.best_response(r["pi_a"][idx], 0, theta, float(g))[1]
                out["v_b"][c0 + idx] = b.best_response(r["pi_b"][idx], 1, theta, float(g))[1]
        out["gap"] = out["v_b"] - out["v_a"]
        return out

    def load(self, Q=None, V=None, pi_a=None, pi_b=None, alpha=None, steps=None, first=0):
        """Resume members first .. first + count - 1 from a checkpoint (count is what the arrays hold; None = unchanged):
        Q[count, nS, 5, 5] and V[count, nS] in [-1, 1], pi_a / pi_b [count, nS, 5], alpha[count], steps for the population.  Q
        alone: V and the strategies of every live state of the range are re-solved on the device.  With V, pi_a and pi_b
        they are stored as given, so with what read() gave a fresh population continues bit for bit.  A refused load changes
        nothing."""
        b = self.batch
        keep = {k: np.ascontiguousarray(x, np.float64) for k, x in zip(self._ROWS + ("alpha",), (Q, V, pi_a, pi_b, alpha)) if x is not None}
        counts = {x.shape[0] for x in keep.values() if x.ndim >= 1}
        assert len(counts) <= 1 and all(x.ndim >= 1 for x in keep.values()), "the arrays must hold the same number of members"
        first, count = self._range(first, counts.pop() if counts else 0)
        shapes = {"Q": (count, self.nS, 5, 5), "V": (count, self.nS), "pi_a": (count, self.nS, 5), "pi_b": (count, self.nS, 5), "alpha": (count,)}
        for k, x in keep.items():
            assert x.shape == shapes[k], "%s must be %s" % (k, list(shapes[k]))
            if k in ("Q", "V"):
                assert (np.abs(x[:, 1:]) <= 1.0).all(), "%s must lie in [-1, 1]" % k
            elif k == "alpha":
                assert ((x >= 0.0) & (x <= 1.0)).all(), "alpha must be [count] values in [0, 1]"
        st = None if steps is None else C.byref(C.c_uint64(int(steps)))
        b._check(b.lib.soccer_minimax_q_population_load(b.h, self.q, first, count,
                                                        *[keep[k].ctypes.data if k in keep else None for k in self._ROWS + ("alpha",)], st))
        return self


class GradientPlay(_Learner):
    """Gradient play on a two-player SoccerBatch (include/soccer_hip.h, "gradient play"): n_a policies of player A and n_b of
    player B live on the device; a step solves policy_gradient's exact gradients of the resident policies against each other's
    weighted mixture and moves every row of every policy along them, projected back onto the simplex.  Nothing is sampled: the
    lanes are left alone and no tick is consumed.  optimism 1 is the optimistic (predictive) step g + (g - previous g)."""
    _C = "soccer_gradient_play"

    def __init__(self, batch, n_a, n_b, discount_factor, eta_a=1.0, eta_b=1.0, optimism=0.0, normalize=True, theta=1e-10,
                 max_sweeps=1000000, pairs_per_pass=0, pi_a=None, pi_b=None):
        nS = batch.nS
        keep = []
        for p, n, name in ((pi_a, n_a, "pi_a"), (pi_b, n_b, "pi_b")):
            if p is not None:
                p = np.ascontiguousarray(p, np.float64)
                p = p[None] if p.ndim == 2 else p
                assert p.shape == (n, nS, 5), "%s must be [%d, n_states, 5]" % (name, n)
            keep.append(p)
        cfg = _lib.GradientPlayConfig(int(n_a), int(n_b), float(eta_a), float(eta_b), float(optimism), float(discount_factor),
                                      float(theta), int(bool(normalize)), int(max_sweeps), int(pairs_per_pass), 0,
                                      None if keep[0] is None else keep[0].ctypes.data, None if keep[1] is None else keep[1].ctypes.data)
        self._create(batch, cfg)
        del keep
        self.n_a, self.n_b, self.discount_factor, self.theta = int(n_a), int(n_b), float(discount_factor), float(theta)

    def run(self, n_steps, trace=False):
        """n_steps steps.  With trace=True returns [n_steps, n_a, n_b]: each step's payoff matrix before its update.  RuntimeError
        if a step's solves are still open at max_sweeps: that step is not applied, steps counts the completed ones (its .results
        holds the trace so far, the rest zeros)."""
        b = self.batch
        tr = np.zeros((int(n_steps), self.n_a, self.n_b)) if trace else None
        code = b.lib.soccer_gradient_play_run(b.h, self.q, int(n_steps), tr.ctypes.data if trace else None)
        try:
            b._check(code)
        except RuntimeError as e:
            e.results = tr
            raise
        return tr if trace else self

    def read(self):
        """dict: pi_a[n_a, nS, 5], pi_b[n_b, nS, 5], prev_a, prev_b (the last step's gradients), w_a[n_a], w_b[n_b], payoff
        [n_a, n_b] (the last step's, before its update) and steps."""
        b, nS = self.batch, self.nS
        out = {"pi_a": np.zeros((self.n_a, nS, 5)), "pi_b": np.zeros((self.n_b, nS, 5)), "prev_a": np.zeros((self.n_a, nS, 5)),
               "prev_b": np.zeros((self.n_b, nS, 5)), "w_a": np.zeros(self.n_a), "w_b": np.zeros(self.n_b),
               "payoff": np.zeros((self.n_a, self.n_b))}
        st = C.c_int64()
        b._check(b.lib.soccer_gradient_play_read(b.h, self.q, *[out[k].ctypes.data for k in
                                                                ("pi_a", "pi_b", "prev_a", "prev_b", "w_a", "w_b", "payoff")], C.byref(st)))
        out["steps"] = int(st.value)
        return out

    def load(self, pi_a=None, pi_b=None, prev_a=None, prev_b=None, payoff=None, steps=None, **ignored):
        """Resume from read()'s dict (load(**learner.read())): a fresh learner continues bit for bit; the weights go through
        weights().  None leaves a part as it is."""
        b, nS = self.batch, self.nS
        arrs = []
        for p, n, name in ((pi_a, self.n_a, "pi_a"), (pi_b, self.n_b, "pi_b"), (prev_a, self.n_a, "prev_a"), (prev_b, self.n_b, "prev_b")):
            if p is not None:
                p = np.ascontiguousarray(p, np.float64)
                assert p.shape == (n, nS, 5), "%s must be [%d, n_states, 5]" % (name, n)
            arrs.append(p)
        if payoff is not None:
            payoff = np.ascontiguousarray(payoff, np.float64)
            assert payoff.shape == (self.n_a, self.n_b), "payoff must be [n_a, n_b]"
        arrs.append(payoff)
        st = None if steps is None else C.byref(C.c_int64(int(steps)))
        b._check(b.lib.soccer_gradient_play_load(b.h, self.q, *[None if p is None else p.ctypes.data for p in arrs], st))
        return self

    def weights(self, w_a=None, w_b=None):
        """Sets the mixtures the policies are trained against from the next step on: w_b [n_b] weighs player A's opponents, w_a
        [n_a] player B's; None is uniform."""
        b = self.batch
        wa, wb = b._weights(w_a, self.n_a, "w_a"), b._weights(w_b, self.n_b, "w_b")
        b._check(b.lib.soccer_gradient_play_set_weights(b.h, self.q, None if wa is None else wa.ctypes.data,
                                                        None if wb is None else wb.ctypes.data))
        return self

    def exploitability(self, theta=None):
        """planners.exploitability of the current sets at the learner's discount: policy i of A with policy i of B (the sets
        must be equally large, or one of them a single policy)."""
        from . import planners
        assert self.n_a == self.n_b or 1 in (self.n_a, self.n_b), "exploitability pairs policy i of A with policy i of B"
        r = self.read()
        return planners.exploitability(self.batch, r["pi_a"], r["pi_b"], self.theta if theta is None else theta, self.discount_factor)

    def cross_play(self, theta=None):
        """planners.cross_play's dict of the current sets at the learner's discount"""
        from . import planners
        r = self.read()
        return planners.cross_play(self.batch, r["pi_a"], r["pi_b"], self.theta if theta is None else theta, self.discount_factor)

    def meta_game(self, theta=None, max_pivots=None):
        """planners.meta_game's dict of the current sets at the learner's discount"""
        from . import planners
        r = self.read()
        return planners.meta_game(self.batch, r["pi_a"], r["pi_b"], self.theta if theta is None else theta, self.discount_factor,
                                  max_pivots=max_pivots)


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
        try:
            self._check(code)
        except RuntimeError as e:               # not converged (or a capture): what was reached goes with the exception
            e.results = (pa, pb, V, Q, int(it.value))
            raise
        return pa, pb, V, Q, int(it.value)

    # -- best responses to mixed policies (two-player handles) ----------------------------------------
    def _policies(self, policy, name):
        """[nS, 5] or [P, nS, 5] -> (contiguous float64 [P, nS, 5], whether a leading axis was given)"""
        p = np.ascontiguousarray(policy, np.float64)
        assert p.ndim in (2, 3) and p.shape[-2:] == (self.nS, 5), "%s must be [n_states, 5] or [P, n_states, 5]" % name
        return (p if p.ndim == 3 else p[None]), p.ndim == 3

    def _response_result(self, code, out, batched):
        out = tuple(x if batched else x[0] for x in out[:-1]) + (out[-1].astype(np.int64) if batched else int(out[-1][0]),)
        try:
            self._check(code)
        except RuntimeError as e:               # not converged (or a capture): what was reached goes with the exception
            e.results = out
            raise
        return out

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
        a, ba = self._policies(pi_a, "pi_a")
        b, bb = self._policies(pi_b, "pi_b")
        n = max(a.shape[0], b.shape[0])
        assert a.shape[0] in (1, n) and b.shape[0] in (1, n), "pi_a and pi_b must hold one policy or the same number of policies"
        a = np.ascontiguousarray(np.broadcast_to(a, (n, self.nS, 5))); b = np.ascontiguousarray(np.broadcast_to(b, (n, self.nS, 5)))
        V = np.zeros((n, self.nS)); it = np.zeros(n, np.int32)
        code = self.lib.soccer_evaluate_policies(self.h, n, a.ctypes.data, b.ctypes.data, float(theta), float(discount_factor),
                                                 int(max_sweeps), V.ctypes.data, it.ctypes.data)
        return self._response_result(code, (V, it), ba or bb)

    def cross_play(self, pi_a, pi_b, theta, discount_factor, max_sweeps=1000000, pairs_per_pass=0, values=False):
        """The payoff matrix of two sets of mixed policies: payoff[i, j] is player A's value at kick-off (the mean of V over the
        initial states) when pi_a[i] meets pi_b[j], each pair iterated exactly like evaluate_policies on that pair alone.
        pi_a is [n_a, nS, 5], pi_b [n_b, nS, 5], up to 1024 policies each (a single [nS, 5] policy is a batch of one).
        Returns (payoff[n_a, n_b], iterations[n_a, n_b]), and with values=True also V[n_a, n_b, nS].  pairs_per_pass: how many
        pairs are solved together on the device (0: the library chooses; else a multiple of 64) — no result depends on it.
        RuntimeError if max_sweeps is reached (its .results holds the tuple, iterations == max_sweeps marks the open pairs)."""
        a, _ = self._policies(pi_a, "pi_a")
        b, _ = self._policies(pi_b, "pi_b")
        na, nb = a.shape[0], b.shape[0]
        payoff = np.zeros((na, nb)); it = np.zeros((na, nb), np.int32)
        V = np.zeros((na, nb, self.nS)) if values else None
        code = self.lib.soccer_cross_play(self.h, na, a.ctypes.data, nb, b.ctypes.data, float(theta), float(discount_factor),
                                          int(max_sweeps), int(pairs_per_pass), payoff.ctypes.data,
                                          V.ctypes.data if values else None, it.ctypes.data)
        out = (payoff, it.astype(np.int64)) + ((V,) if values else ())
        try:
            self._check(code)
        except RuntimeError as e:               # not converged (or a capture): what was reached goes with the exception
            e.results = out
            raise
        return out

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
        a, _ = self._policies(pi_a, "pi_a")
        b, _ = self._policies(pi_b, "pi_b")
        na, nb = a.shape[0], b.shape[0]
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
        try:
            self._check(code)
        except RuntimeError as e:               # not converged (or a capture): what was reached goes with the exception
            e.results = out
            raise
        return out

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
        a, _ = self._policies(pi_a, "pi_a")
        b, _ = self._policies(pi_b, "pi_b")
        na, nb = a.shape[0], b.shape[0]
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
        try:
            self._check(code)
        except RuntimeError as e:               # not converged (or a capture): what was reached goes with the exception
            e.results = out
            raise
        return out

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
        a, _ = self._policies(pi_a, "pi_a")
        b, _ = self._policies(pi_b, "pi_b")
        na, nb, nS = a.shape[0], b.shape[0], self.nS
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
        try:
            self._check(code)
        except RuntimeError as e:               # not converged (or a capture): what was reached goes with the exception
            e.results = out
            raise
        return out

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
        try:
            self._check(code)
        except RuntimeError as e:               # a game stopped at the cap (or a capture): what was reached goes with the exception
            e.results = out
            raise
        return out

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
