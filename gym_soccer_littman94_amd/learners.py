"""The learners of a SoccerBatch: thin wrappers over the C learners of libsoccer_hip.so (include/soccer_hip.h, "learners").

Every wrapper sits on _Learner, the populations on _Population.  A class says what is its own: its C prefix (_C), its
fields in the C argument order of its read and load (_FIELDS), whether those take the fields as positional pointers or in a
state struct (_STATE), and the policy pairs it can be evaluated on (_WHICH).  read, load, the alpha / steps / dscale
properties, exploitability and the pair evaluators all come from those ("the Python layer").  The config
functions check a learner's parameters before any library call and build its C config.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._device import DeviceArray, _ptr

DECAY = 0.01 ** (1 / 1e6)       # the default decay: alpha falls to 1 % over a million steps
_S = "nS"                       # the number of states, in a field's shape
_ROWS = (_S, 5)                 # a table of one row of five per state

# -- hyperparameters: name -> (predicate on a float or an array, the range in words) ---------------------------------
_UNIT = (lambda x: (0.0 <= x) & (x <= 1.0), "[0, 1]")
_RATE = (lambda x: (0.0 < x) & (x <= 1.0), "(0, 1]")
_HYPER = {"discount_factor": (lambda x: (0.0 <= x) & (x < 1.0), "[0, 1)"), "alpha": _UNIT, "decay": _RATE, "explor": _UNIT,
          "q_init": (lambda x: (-1.0 <= x) & (x <= 1.0), "[-1, 1]"), "delta_win": _UNIT, "delta_lose": _UNIT, "delta_decay": _RATE}

# -- how a player acts: (the strings and their constants, the constant of a fixed policy) ----------------------------
_MQ_KINDS = ({"uniform": _lib.MQ_UNIFORM, "self": _lib.MQ_SELF}, _lib.MQ_FIXED)
_QL_KINDS = ({"greedy": _lib.QL_GREEDY, "uniform": _lib.QL_UNIFORM}, _lib.QL_FIXED)
_PHC_KINDS = ({"learn": _lib.PHC_LEARN, "uniform": _lib.PHC_UNIFORM}, _lib.PHC_FIXED)


def _scalar(name, value):
    """a hyperparameter as a float, AssertionError outside its range"""
    x = float(value)
    assert _HYPER[name][0](x), "%s must be in %s" % (name, _HYPER[name][1])
    return x


def _per_member(name, value, n):
    """A hyperparameter that is a scalar for every member or an array of n, one value per member: (scalar, array or None);
    with an array the scalar is its first value."""
    if np.ndim(value) == 0:
        return _scalar(name, value), None
    a = np.ascontiguousarray(value, np.float64)
    assert a.shape == (int(n),), "a per-member %s must have one value per lane (%d)" % (name, n)
    assert _HYPER[name][0](a).all(), "every per-member %s must be in %s" % (name, _HYPER[name][1])
    return float(a[0]), a


def _scalars(**given):
    return [_scalar(name, value) for name, value in given.items()]


def _members(n, **given):
    """_per_member of each: ({name: scalar}, {name: array or None})"""
    both = {name: _per_member(name, value, n) for name, value in given.items()}
    return {k: v[0] for k, v in both.items()}, {k: v[1] for k, v in both.items()}


def _kind(name, value, kinds, nS, n=None, where=False):
    """A kind given as a string, or a fixed policy: (the kind's constant, the [nS, 5] policy or None, the [n, nS, 5] policy of
    a fixed policy per member or None).  kinds: (the allowed strings and their constants, the constant of a fixed policy);
    n: the members of a population that takes a policy per member, None where there is no such thing; where: the message says
    which row is not a distribution."""
    strings, fixed = kinds
    if isinstance(value, str):
        assert value in strings, "%s must be %s%s mixed policy" % (
            name, ", ".join(repr(s) for s in strings), " or an [nS, 5]" if n is None else ", an [nS, 5] or an [n, nS, 5]")
        return strings[value], None, None
    must = "a fixed %s must be %s rows" % (name, "[n_states, 5]" if n is None else "[n_states, 5] or [n_lanes, n_states, 5]")
    pol = np.ascontiguousarray(value, np.float64)
    assert pol.shape == (int(nS), 5) or (n is not None and pol.shape == (int(n), int(nS), 5)), must + " summing to 1"
    bad = np.argwhere(~((pol >= 0).all(-1) & np.isclose(pol.sum(-1), 1.0)))
    if len(bad):
        assert where, must + " summing to 1"
        row = "state %d" % bad[0][0] if pol.ndim == 2 else "member %d, state %d" % tuple(bad[0])
        raise AssertionError(must + " >= 0 summing to 1: %s is not" % row)
    return fixed, (pol if pol.ndim == 2 else None), (pol if pol.ndim == 3 else None)


def _data(x):
    return None if x is None else x.ctypes.data


def minimax_q_config(nS, discount_factor, alpha=1.0, decay=DECAY, explor=0.2, q_init=1.0, opponent="uniform"):
    """Checks the parameters of a minimax-Q learner (AssertionError, before any library call) and returns
    (soccer_minimax_q_config, the array it points into or None)."""
    hyper = _scalars(discount_factor=discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init)
    kind, pol, _ = _kind("opponent", opponent, _MQ_KINDS, nS)
    return _lib.MinimaxQConfig(*hyper, kind, 0, _data(pol)), pol


def q_learning_config(nS, discount_factor, alpha=1.0, decay=DECAY, explor=0.2, q_init=1.0, act_a="greedy", act_b="greedy"):
    """Checks the parameters of the independent Q-learners (AssertionError, before any library call) and returns
    (soccer_q_learner_config, the arrays it points into)."""
    hyper = _scalars(discount_factor=discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init)
    (kind_a, pol_a, _), (kind_b, pol_b, _) = _kind("act_a", act_a, _QL_KINDS, nS), _kind("act_b", act_b, _QL_KINDS, nS)
    return _lib.QLearnerConfig(*hyper, kind_a, kind_b, _data(pol_a), _data(pol_b)), [pol_a, pol_b]


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


def q_population_config(n, nS, discount_factor, alpha=1.0, decay=DECAY, explor=0.2, q_init=1.0, act_a="greedy", act_b="greedy",
                        league=None):
    """Checks the parameters of a population of Q-learners (AssertionError, before any library call) and returns
    (soccer_q_population_config, the arrays it points into).  discount_factor, alpha, decay and explor are scalars for every
    member or arrays of n, one value per member.  league: league_config's tuple, or None; its player is SOCCER_QL_FIXED
    with a NULL policy in the config."""
    if league is not None:                      # (the other checks see a placeholder for the league's player)
        act_a, act_b = ("uniform", act_b) if league[0] == 0 else (act_a, "uniform")
    s, arrays = _members(n, discount_factor=discount_factor, alpha=alpha, decay=decay, explor=explor)
    # (the scalar checks of q_learning_config hold for the kinds, the fixed policies and q_init)
    base, pols = q_learning_config(nS, s["discount_factor"], s["alpha"], s["decay"], s["explor"], q_init, act_a, act_b)
    cfg = _lib.QPopulationConfig(*[getattr(base, name) for name, _ in base._fields_],
                                 *[_data(arrays[k]) for k in ("alpha", "decay", "explor", "discount_factor")])
    if league is not None:
        setattr(cfg, "act_b" if league[0] else "act_a", _lib.QL_FIXED)
    return cfg, (pols, arrays)


def om_population_config(n, nS, discount_factor, alpha=1.0, decay=DECAY, explor=0.2, q_init=1.0, act_a="greedy", act_b="greedy"):
    """Checks the parameters of a population of opponent-modelling Q-learners (AssertionError, before any library call) and
    returns (soccer_om_population_config, the arrays it points into): q_population_config's checks and layout, no league."""
    cfg, keep = q_population_config(n, nS, discount_factor, alpha, decay, explor, q_init, act_a, act_b)
    return _lib.OMPopulationConfig.from_buffer_copy(cfg), keep


def wolf_phc_config(nS, discount_factor, alpha=1.0, decay=DECAY, explor=0.2, q_init=1.0, delta_win=0.01, delta_lose=0.04,
                    delta_decay=1.0, act_a="learn", act_b="learn"):
    """Checks the parameters of the policy hill-climbers (AssertionError, before any library call) and returns
    (soccer_wolf_phc_config, the arrays it points into)."""
    hyper = _scalars(discount_factor=discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init, delta_win=delta_win,
                     delta_lose=delta_lose, delta_decay=delta_decay)
    (kind_a, pol_a, _), (kind_b, pol_b, _) = _kind("act_a", act_a, _PHC_KINDS, nS), _kind("act_b", act_b, _PHC_KINDS, nS)
    return _lib.WolfPHCConfig(*hyper, kind_a, kind_b, _data(pol_a), _data(pol_b)), [pol_a, pol_b]


def wolf_population_config(n, nS, discount_factor, alpha=1.0, decay=DECAY, explor=0.2, q_init=1.0, delta_win=0.01,
                           delta_lose=0.04, delta_decay=1.0, act_a="learn", act_b="learn"):
    """Checks the parameters of a population of policy hill-climbers (AssertionError, before any library call) and returns
    (soccer_wolf_population_config, the arrays it points into).  The seven hyperparameters are scalars for every member or
    arrays of n, one value per member; act_a / act_b: 'learn', 'uniform', one fixed [nS, 5] mixed policy for every member, or
    [n, nS, 5], a fixed policy per member."""
    s, arrays = _members(n, discount_factor=discount_factor, alpha=alpha, decay=decay, explor=explor, delta_win=delta_win,
                         delta_lose=delta_lose, delta_decay=delta_decay)
    q0 = _scalar("q_init", q_init)
    kinds, shared, each = zip(_kind("act_a", act_a, _PHC_KINDS, nS, n), _kind("act_b", act_b, _PHC_KINDS, nS, n))
    cfg = _lib.WolfPopulationConfig(s["discount_factor"], s["alpha"], s["decay"], s["explor"], q0, s["delta_win"], s["delta_lose"],
                                    s["delta_decay"], *kinds, *[_data(x) for x in shared + each],
                                    *[_data(arrays[k]) for k in ("alpha", "decay", "explor", "discount_factor", "delta_win", "delta_lose",
                                                                 "delta_decay")])
    return cfg, ((list(shared), list(each)), arrays)


def regret_population_config(n, nS, discount_factor, alpha=1.0, decay=DECAY, explor=0.2, q_init=1.0, plus=True, linear=False,
                             act_a="learn", act_b="learn"):
    """Checks the parameters of a population of regret matchers (AssertionError, before any library call) and returns
    (soccer_regret_population_config, the arrays it points into).  discount_factor, alpha, decay and explor are scalars for
    every member or arrays of n, one value per member; plus and linear are flags of the whole population; act_a / act_b:
    'learn', 'uniform', one fixed [nS, 5] mixed policy for every member, or [n, nS, 5], a fixed policy per member."""
    s, arrays = _members(n, discount_factor=discount_factor, alpha=alpha, decay=decay, explor=explor)
    q0 = _scalar("q_init", q_init)
    for name, flag in (("plus", plus), ("linear", linear)):
        assert isinstance(flag, (bool, np.bool_)) or flag in (0, 1), "%s must be True or False" % name
    kinds, shared, each = zip(_kind("act_a", act_a, _PHC_KINDS, nS, n, where=True), _kind("act_b", act_b, _PHC_KINDS, nS, n, where=True))
    cfg = _lib.RegretPopulationConfig(s["discount_factor"], s["alpha"], s["decay"], s["explor"], q0, *kinds, int(bool(plus)),
                                      int(bool(linear)), *[_data(x) for x in shared + each],
                                      *[_data(arrays[k]) for k in ("alpha", "decay", "explor", "discount_factor")])
    return cfg, ((list(shared), list(each)), arrays)


def _flags(**given):
    for name, flag in given.items():
        assert isinstance(flag, (bool, np.bool_)) or flag in (0, 1), "%s must be True or False" % name
    return [int(bool(flag)) for flag in given.values()]


def regret_learner_config(nS, discount_factor, alpha=1.0, decay=DECAY, explor=0.2, q_init=1.0, plus=True, linear=False,
                          act_a="learn", act_b="learn"):
    """Checks the parameters of the regret matchers of one table (AssertionError, before any library call) and returns
    (soccer_regret_learner_config, the arrays it points into).  plus: regret matching+; linear: linear averaging; act_a /
    act_b: 'learn', 'uniform' or a fixed [nS, 5] mixed policy."""
    hyper = _scalars(discount_factor=discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init)
    flags = _flags(plus=plus, linear=linear)
    (kind_a, pol_a, _), (kind_b, pol_b, _) = (_kind("act_a", act_a, _PHC_KINDS, nS, where=True),
                                              _kind("act_b", act_b, _PHC_KINDS, nS, where=True))
    return _lib.RegretLearnerConfig(*hyper, kind_a, kind_b, *flags, _data(pol_a), _data(pol_b)), [pol_a, pol_b]


def minimax_q_population_config(n, nS, discount_factor, alpha=1.0, decay=DECAY, explor=0.2, q_init=1.0, opponent="uniform"):
    """Checks the parameters of a population of minimax-Q learners (AssertionError, before any library call) and returns
    (soccer_minimax_q_population_config, the arrays it points into).  discount_factor, alpha, decay and explor are scalars
    for every member or arrays of n, one value per member; opponent: 'uniform', 'self', one fixed [nS, 5] mixed policy for
    every member, or [n, nS, 5], a fixed policy per member."""
    s, arrays = _members(n, discount_factor=discount_factor, alpha=alpha, decay=decay, explor=explor)
    q0 = _scalar("q_init", q_init)
    kind, shared, each = _kind("opponent", opponent, _MQ_KINDS, nS, n, where=True)
    cfg = _lib.MinimaxQPopulationConfig(s["discount_factor"], s["alpha"], s["decay"], s["explor"], q0, kind, 0, _data(shared), _data(each),
                                        *[_data(arrays[k]) for k in ("alpha", "decay", "explor", "discount_factor")])
    return cfg, ((shared, each), arrays)


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


def _meta_of_cross_play(batch, payoff, iterations, max_pivots):
    """cross-play's dict (planners.cross_play) plus the solved meta-game and what mixing buys player A"""
    row_min, col_max = payoff.min(1), payoff.max(0)
    out = {"payoff": payoff, "iterations": iterations, "row_min": row_min, "col_max": col_max,
           "bounds": (float(row_min.max()), float(col_max.min()))}
    m = batch.solve_meta_game(payoff, max_pivots=max_pivots)
    out.update({k: m[k] for k in ("x", "y", "value", "lo", "hi", "status")})
    out["gain"] = out["lo"] - out["bounds"][0]
    return out


def _greedy(out):
    """read()'s derived values of Q-learners: V_p the row maxima of Q_p, pi_p the one-hot of the first greedy action"""
    for p in "ab":
        out["V_" + p] = out["Q_" + p].max(-1)
        out["pi_" + p] = np.eye(5)[out["Q_" + p].argmax(-1)]
    return out


def _field(key, doc=None):
    """a property that reads one field of _FIELDS alone (a population: of every member)"""
    return property(lambda self: self._read((key,), *self._everyone(key))[key], doc=doc)


class _Learner:
    """What the wrappers of a C learner share.  A kind states:
      _C       the prefix of its C entry points: _C + "_create", "_run", "_destroy", "_read", "_load"
      _FIELDS  what its read and load take, in the C argument order: (key, shape, dtype).  shape is what follows the members'
               axis of a population, in terms of _S, the number of states; None: one C scalar, passed by pointer, of the
               ctypes type that stands as dtype
      _STATE   the _lib struct its read and load take the fields in; None: they take them as positional pointers
      _LOADS   the keys its load takes, where they are not all of _FIELDS
      _WHICH   the pairs of policies it can be evaluated on: name -> (player A's key, player B's key) of read()
      _PAIRED  load's messages name Q_a and Q_b together and list the arrays (the wording of the kinds that came first)"""
    _C = None
    _FIELDS = ()
    _STATE = None
    _LOADS = None
    _WHICH = {None: ("pi_a", "pi_b")}
    _PAIRED = False

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

    def _update(self, obs, act_a, act_b, reward, terminated, next_obs):
        _learner_update(self.batch, getattr(self.batch.lib, self._C + "_update"), self.q, obs, act_a, act_b, reward, terminated, next_obs)
        return self

    def _dims(self, shape):
        return tuple(self.nS if d == _S else d for d in shape)

    def _everyone(self, key):
        return ()

    def _call(self, what, members, slots, keys):
        """The kind's read or load (`what`) on slots: key -> the numpy array or the ctypes scalar that goes as that argument,
        NULL where there is none.  members: (first, count) of a population; keys: the positional order."""
        def address(x, of):
            return x.ctypes.data if isinstance(x, np.ndarray) else of(x)
        if self._STATE is None:
            args = [address(slots[k], C.byref) if k in slots else None for k in keys]
        else:
            args = [C.byref(self._STATE(**{k: address(x, C.pointer) for k, x in slots.items()}))]
        b = self.batch
        b._check(getattr(b.lib, self._C + what)(b.h, self.q, *members, *args))

    def _read(self, keys=None, *members):
        """the library's own arrays and scalars: those of `keys` (None: all of _FIELDS), of `members` in a population"""
        out = {k: dt() if shape is None else np.zeros(members[1:] + self._dims(shape), dt)
               for k, shape, dt in self._FIELDS if keys is None or k in keys}
        self._call("_read", members, out, [f[0] for f in self._FIELDS])
        return {k: x if isinstance(x, np.ndarray) else x.value for k, x in out.items()}

    def _load(self, given, first=None):
        """load() of `given`, key -> value (None: left as it is), held to _FIELDS before any library call: the shapes, Q and V
        in [-1, 1] (but for row 0, the terminal observation), alpha and dscale in [0, 1].  first: of a population, whose
        arrays hold the same number of members."""
        keep, members = {}, ()
        for k, shape, dt in self._FIELDS:
            if given.get(k) is not None:
                keep[k] = np.ascontiguousarray(given[k], dt) if shape is not None else dt(float(given[k]) if dt is C.c_double else int(given[k]))
        if first is not None:
            counts = {x.shape[0] for x in keep.values() if isinstance(x, np.ndarray) and x.ndim >= 1}
            names = [k for k, shape, _ in self._FIELDS if shape is not None]
            assert len(counts) <= 1, "%s must hold the same number of members" % (
                ", ".join(names[:-1]) + " and " + names[-1] if self._PAIRED else "the arrays")
            members = self._range(first, counts.pop() if counts else 0)
        for k, shape, _ in self._FIELDS:
            x = keep.get(k)
            if x is None:
                continue
            if shape is None:
                assert k not in ("alpha", "dscale") or 0.0 <= x.value <= 1.0, "%s must be in [0, 1]" % k
                continue
            text = "[%s]" % ", ".join(["count"] * len(members[1:]) + ["n_states" if d == _S else str(d) for d in shape])
            if shape == ():                         # (a value per member: alpha and dscale)
                assert x.shape == members[1:] and ((x >= 0.0) & (x <= 1.0)).all(), "%s must be %s values in [0, 1]" % (k, text)
                continue
            both = self._PAIRED and k[-2:] in ("_a", "_b")
            assert x.shape == members[1:] + self._dims(shape), "%s must be %s" % ("%s_a / %s_b" % (k[:-2], k[:-2]) if both else k, text)
            if k[0] in "QV":
                assert (np.abs(x[:, 1:] if members else x[1:]) <= 1.0).all(), "%s must lie in [-1, 1]" % ("Q" if k[0] == "Q" else k)
        self._call("_load", members, keep, self._LOADS or [f[0] for f in self._FIELDS])
        return self

    def _pair(self, which):
        assert which in self._WHICH, "which must be %s" % " or ".join(repr(k) for k in self._WHICH)
        return self._WHICH[which]

    def _exploitability(self, which, theta):
        """planners.exploitability of the pair `which` of read() at the learner's discount"""
        from . import planners
        ka, kb = self._pair(which)
        r = self.read()
        return planners.exploitability(self.batch, r[ka], r[kb], theta, self.discount_factor)


class _Population(_Learner):
    """What the populations share: a member per lane with its own discount, ranges of members, update(), and the evaluations
    of the members' policies: exploitability and the pair evaluators, on the pair `which` of _WHICH."""

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

    def _everyone(self, key):
        return 0, 0 if key == "steps" else self.n

    def _read(self, keys=None, first=0, count=None):
        return super()._read(keys, *self._range(first, count))

    def _policies(self, first, count, keys):
        """read()'s entries `keys` of a range; a kind whose policies are not fields of the library derives them here"""
        return self._read(keys, first, count)

    def _exploitability(self, which, theta, first, count):
        ka, kb = self._pair(which)
        first, count = self._range(first, count)
        b = self.batch
        out = {k: np.zeros((count, self.nS)) for k in ("v_a", "v_b", "gap")}
        for c0 in range(0, count, _lib.BR_MAX_POLICIES):
            c = min(_lib.BR_MAX_POLICIES, count - c0)
            r = self._policies(first + c0, c, (ka, kb))
            gam = self.discount_factor[first + c0:first + c0 + c]
            for g in np.unique(gam):                # (one solve per discount in the chunk: a batch shares its discount)
                idx = np.flatnonzero(gam == g)
                out["v_a"][c0 + idx] = b.best_response(r[ka][idx], 0, theta, float(g))[1]
                out["v_b"][c0 + idx] = b.best_response(r[kb][idx], 1, theta, float(g))[1]
        out["gap"] = out["v_b"] - out["v_a"]
        return out

    def _pairs(self, what, name, which, theta, first, count, discount, **more):
        """SoccerBatch's pair evaluator `what` on members first .. first + count - 1 against one another: player A's policies
        of the pair `which` meet the same members' player-B policies, read in chunks of at most 256 members.  discount None
        (the parameter called `name`): the one the members share, ValueError if they differ."""
        ka, kb = self._pair(which)
        first, count = self._range(first, count)
        assert 1 <= count <= _lib.CROSS_MAX_POLICIES, "%s takes 1 .. %d members, not %d" % (what, _lib.CROSS_MAX_POLICIES, count)
        gam = self.discount_factor[first:first + count]
        if discount is None:
            other = np.flatnonzero(gam != gam[0])
            if other.size:
                raise ValueError("members %d and %d have different discounts (%r and %r): pass %s" % (
                    first, first + other[0], float(gam[0]), float(gam[other[0]]), name))
            discount = float(gam[0])
        pa = np.zeros((count, self.nS, 5)); pb = np.zeros((count, self.nS, 5))
        for c0 in range(0, count, _lib.BR_MAX_POLICIES):
            c = min(_lib.BR_MAX_POLICIES, count - c0)
            r = self._policies(first + c0, c, (ka, kb))
            pa[c0:c0 + c] = r[ka]; pb[c0:c0 + c] = r[kb]
        return getattr(self.batch, what)(pa, pb, theta, float(discount), **more)

    def exploitability(self, theta=1e-10, first=0, count=None):
        """How badly the best possible opponent beats the pair of policies of each member of a range (Q-learners: the one-hot
        greedy policies), at that member's discount: they go through SoccerBatch.best_response in batches of at most 256
        members with one discount.  Returns {"v_a", "v_b", "gap"}, arrays of [count, nS] (planners.exploitability's per
        member)."""
        return self._exploitability(None, theta, first, count)

    def cross_play(self, theta=1e-10, first=0, count=None, discount_factor=None):
        """What each member's player A scores against each member's player B: (payoff[count, count], iterations) of
        SoccerBatch.cross_play on pi_a and pi_b (Q-learners: the one-hot greedy policies) of members first ..
        first + count - 1 (at most 1024).  discount_factor None: the range's common discount, ValueError if the members differ."""
        return self._pairs("cross_play", "discount_factor", None, theta, first, count, discount_factor)

    def meta_game(self, theta=1e-10, first=0, count=None, discount_factor=None, max_pivots=None):
        """cross_play with the same arguments, then its meta-game solved (planners.meta_game): the members' mixture a rational
        opponent cannot beat, x, y, value, lo, hi, status, and gain = lo - the best single member's row_min."""
        return _meta_of_cross_play(self.batch, *self.cross_play(theta, first, count, discount_factor), max_pivots)

    def match_outcomes(self, theta=1e-10, first=0, count=None, continue_prob=None):
        """How often each member's player A beats each member's player B, how often they draw and how long they play:
        SoccerBatch.match_outcomes' dict on cross_play's policies of members first .. first + count - 1 (at most 1024).
        continue_prob None: the range's common discount, ValueError if the members differ."""
        return self._pairs("match_outcomes", "continue_prob", None, theta, first, count, continue_prob)

    def occupancy(self, theta=1e-10, first=0, count=None, continue_prob=None, features=None, values=False):
        """Where each member's player A and each member's player B play their game: SoccerBatch.occupancy's dict on cross_play's
        policies of members first .. first + count - 1 (at most 1024).  continue_prob None: the range's common discount,
        ValueError if the members differ."""
        return self._pairs("occupancy", "continue_prob", None, theta, first, count, continue_prob, features=features, values=values)


def _population_with_a_choice(default):
    """_Population for a kind with more than one pair of policies to evaluate: the five evaluations take `which`, a name of
    the kind's _WHICH, as their first parameter, `default` where it is not given."""
    class Choice(_Population):
        def exploitability(self, which=default, theta=1e-10, first=0, count=None):
            return self._exploitability(which, theta, first, count)

        def cross_play(self, which=default, theta=1e-10, first=0, count=None, discount_factor=None):
            return self._pairs("cross_play", "discount_factor", which, theta, first, count, discount_factor)

        def meta_game(self, which=default, theta=1e-10, first=0, count=None, discount_factor=None, max_pivots=None):
            return _meta_of_cross_play(self.batch, *self.cross_play(which, theta, first, count, discount_factor), max_pivots)

        def match_outcomes(self, which=default, theta=1e-10, first=0, count=None, continue_prob=None):
            return self._pairs("match_outcomes", "continue_prob", which, theta, first, count, continue_prob)

        def occupancy(self, which=default, theta=1e-10, first=0, count=None, continue_prob=None, features=None, values=False):
            return self._pairs("occupancy", "continue_prob", which, theta, first, count, continue_prob, features=features, values=values)

    for name in ("exploitability", "cross_play", "meta_game", "match_outcomes", "occupancy"):
        getattr(Choice, name).__doc__ = getattr(_Population, name).__doc__ + \
            "\n        which: the pair of policies that is evaluated, a name of the class's _WHICH (its docstring says what they are)."
    return Choice


class MinimaxQLearner(_Learner):
    """A minimax-Q learner (Littman 1994) on a two-player auto-reset SoccerBatch: one shared Q[nS, 5, 5] on the device,
    the batch's lanes as actors (include/soccer_hip.h, "learners").  run() enqueues and returns; the properties
    synchronise and copy."""
    _C = "soccer_minimax_q"
    _FIELDS = (("Q", (_S, 5, 5), np.float64), ("V", (_S,), np.float64), ("pi_a", _ROWS, np.float64), ("pi_b", _ROWS, np.float64),
               ("visits", (_S, 25), np.uint64), ("alpha", None, C.c_double), ("steps", None, C.c_uint64))
    _LOADS = ("Q", "visits", "alpha", "steps")

    def __init__(self, batch, discount_factor, **params):
        cfg, keep = minimax_q_config(batch.nS, discount_factor, **params)
        self._create(batch, cfg)
        del keep                                   # (create has copied the opponent's thresholds)
        self.discount_factor = float(discount_factor)

    def update(self, obs, act_a, act_b, reward, terminated, next_obs):
        """One learner step's reduce / update / re-solve on a batch of transitions: DeviceArrays (or device tensors) of one
        length, or numpy arrays, which are copied to the device first."""
        return self._update(obs, act_a, act_b, reward, terminated, next_obs)

    def read(self):
        """dict: Q[nS, 5, 5], V[nS], pi_a / pi_b [nS, 5], visits[nS, 25], alpha, steps (synchronises)."""
        return self._read()

    Q, V, pi_a, pi_b, visits = _field("Q"), _field("V"), _field("pi_a"), _field("pi_b"), _field("visits")
    alpha, steps = _field("alpha"), _field("steps")

    def exploitability(self, theta=1e-10):
        """How badly the best possible opponent beats the strategies the learner holds now, at its discount:
        planners.exploitability of (pi_a, pi_b).  Synchronises and copies; run() does not."""
        return self._exploitability(None, theta)

    def load(self, Q, visits=None, alpha=None, steps=None):
        """Resume from a checkpoint: Q[nS, 5, 5] in, V and the strategies re-solved on the device.  With `visits` (and the
        `alpha` / `steps` of read()) a fresh learner continues bit for bit; without, every state is solved."""
        return self._load(dict(Q=Q, visits=visits, alpha=alpha, steps=steps))


class QLearner(_Learner):
    """Independent Q-learners for both players (Littman 1994's baseline and challenger) on a two-player auto-reset
    SoccerBatch: Q_a[nS, 5] and Q_b[nS, 5] (player B's in its own reward) on the device, the batch's lanes as actors
    (include/soccer_hip.h, "learners, independent Q").  run() enqueues and returns; read() and the properties synchronise
    and copy."""
    _C = "soccer_q_learner"
    _FIELDS = (("Q_a", _ROWS, np.float64), ("Q_b", _ROWS, np.float64), ("visits", (_S, 25), np.uint64), ("alpha", None, C.c_double),
               ("steps", None, C.c_uint64))
    _PAIRED = True

    def __init__(self, batch, discount_factor, **params):
        cfg, keep = q_learning_config(batch.nS, discount_factor, **params)
        self._create(batch, cfg)
        del keep                                   # (create has copied the fixed policies' thresholds)
        self.discount_factor = float(discount_factor)

    def update(self, obs, act_a, act_b, reward, terminated, next_obs):
        """One learner step's reduce / update on a batch of transitions (reward is player A's): DeviceArrays (or device
        tensors) of one length, or numpy arrays, which are copied to the device first."""
        return self._update(obs, act_a, act_b, reward, terminated, next_obs)

    def read(self):
        """dict: Q_a / Q_b [nS, 5], V_a / V_b [nS] (the row maxima), pi_a / pi_b [nS, 5] (one-hot of the first greedy action:
        they plug into rollout(mixed_policies=...) and planners.exploitability as they are; row 0, the terminal observation,
        is whatever argmax of zeros gives and is never read), visits[nS, 25], alpha, steps.  Synchronises."""
        return _greedy(self._read())

    alpha, steps = _field("alpha"), _field("steps")

    def exploitability(self, theta=1e-10):
        """How badly the best possible opponent beats the greedy pair the learners hold now, at their discount:
        planners.exploitability of (pi_a, pi_b).  Synchronises and copies; run() does not."""
        return self._exploitability(None, theta)

    def load(self, Q_a, Q_b, visits=None, alpha=None, steps=None):
        """Resume from a checkpoint: Q_a / Q_b [nS, 5] in; everything derived from them is recomputed on the device.  With
        the `visits`, `alpha` and `steps` of read() a fresh learner continues bit for bit; without `visits` the counts are
        zeroed."""
        return self._load(dict(Q_a=Q_a, Q_b=Q_b, visits=visits, alpha=alpha, steps=steps))


class QPopulation(_Population):
    """A population of independent Q-learners on a two-player auto-reset SoccerBatch, a learner per lane: member i has its own
    Q_a[nS, 5], Q_b[nS, 5] and alpha and learns from lane i alone (include/soccer_hip.h, "learners, a population of
    independent Q-learners").  run() enqueues and returns; read() and the properties synchronise and copy.  Whole populations
    run to gigabytes, so read(), load() and exploitability() take a range of members."""
    _C = "soccer_q_population"
    _FIELDS = (("Q_a", _ROWS, np.float64), ("Q_b", _ROWS, np.float64), ("alpha", (), np.float64), ("steps", None, C.c_uint64))
    _PAIRED = True

    def __init__(self, batch, discount_factor, league_policies=None, league_weights=None, **params):
        lg = league_config(batch.nS, params.get("act_a", "greedy"), params.get("act_b", "greedy"), league_policies, league_weights)
        cfg, keep = q_population_config(batch.n, batch.nS, discount_factor, league=lg, **params)
        self.league, self.n_policies = (None, 0) if lg is None else lg[:2]      # the league's player (0 = A, 1 = B) and its K
        self._create(batch, cfg, keep[1], *(() if lg is None else (lg[0], lg[1], lg[2].ctypes.data, lg[3].ctypes.data)))
        del keep                                   # (create has copied the parameters and the fixed policies' thresholds)

    def _policies(self, first, count, keys):
        return self.read(first, count)

    def read(self, first=0, count=None):
        """dict for members first .. first + count - 1 (count None: to the end): Q_a / Q_b [count, nS, 5], V_a / V_b
        [count, nS] (the row maxima), pi_a / pi_b [count, nS, 5] (one-hot of the first greedy action), alpha[count], steps.
        Synchronises."""
        return _greedy(self._read(None, first, count))

    alpha, steps = _field("alpha", "every member's learning rate, [n]"), _field("steps")

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
        return self._load(dict(Q_a=Q_a, Q_b=Q_b, alpha=alpha, steps=steps), first)


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


class OpponentModelPopulation(_population_with_a_choice("greedy")):
    """A population of opponent-modelling Q-learners (joint-action learners; fictitious play in self-play) on a two-player
    auto-reset SoccerBatch, a learner per lane: member i has, per player, a joint-action table Q[nS, 5, 5] over (own action,
    the other's action) in that player's own reward and the counts C[nS, 5] of the other player's actions, and its alpha, and
    learns from lane i alone (include/soccer_hip.h, "learners, a population of opponent-modelling Q-learners").  A player
    answers the other's empirical frequencies greedily.  run() enqueues and returns; read() and the properties synchronise and
    copy.  read(), load() and exploitability() take a range of members (a member is 390 KB on 5x4).  The evaluations take
    which='greedy', the pair of greedy policies, or which='model', the pair of models (model_a, what B has seen A play, with
    model_b)."""
    _C = "soccer_om_population"
    _FIELDS = (("Q_a", (_S, 5, 5), np.float64), ("Q_b", (_S, 5, 5), np.float64), ("C_a", _ROWS, np.uint64), ("C_b", _ROWS, np.uint64),
               ("alpha", (), np.float64), ("steps", None, C.c_uint64))
    _WHICH = {"greedy": ("pi_a", "pi_b"), "model": ("model_a", "model_b")}
    _PAIRED = True

    def __init__(self, batch, discount_factor, **params):
        cfg, keep = om_population_config(batch.n, batch.nS, discount_factor, **params)
        self._create(batch, cfg, keep[1])
        del keep                                   # (create has copied the parameters and the fixed policies' thresholds)

    def _policies(self, first, count, keys):
        return self.read(first, count)

    def read(self, first=0, count=None):
        """dict for members first .. first + count - 1 (count None: to the end): Q_a / Q_b [count, nS, 5, 5], C_a / C_b
        [count, nS, 5] (uint64), alpha[count], steps; and, computed here by the definition's expression, V_a / V_b [count, nS]
        and pi_a / pi_b [count, nS, 5] (one-hot of g); and model_a = C_b as frequencies (what B has seen A play; 0.2 where
        nothing was seen), model_b = C_a likewise.  Synchronises."""
        out = self._read(None, first, count)
        for p, other in (("a", "b"), ("b", "a")):
            out["V_" + p], g = om_derive(out["Q_" + p], out["C_" + p])
            out["pi_" + p] = np.eye(5)[g]
            out["model_" + p] = om_model(out["C_" + other])
        return out

    alpha, steps = _field("alpha", "every member's learning rate, [n]"), _field("steps")

    def load(self, Q_a=None, Q_b=None, C_a=None, C_b=None, alpha=None, steps=None, first=0):
        """Resume members first .. first + count - 1 from a checkpoint (count is what the arrays hold; None = unchanged): Q_a /
        Q_b [count, nS, 5, 5] in [-1, 1], C_a / C_b [count, nS, 5] counts, alpha[count], steps for the population.  V and the
        greedy actions follow on the device.  With what read() gave, a fresh population continues bit for bit.  A refused
        load changes nothing."""
        return self._load(dict(Q_a=Q_a, Q_b=Q_b, C_a=C_a, C_b=C_b, alpha=alpha, steps=steps), first)


_WOLF_TABLES = tuple((k, _ROWS, np.float64) for k in ("Q_a", "Q_b", "pi_a", "pi_b", "avg_a", "avg_b"))
_WOLF_WHICH = {"pi": ("pi_a", "pi_b"), "avg": ("avg_a", "avg_b")}


def _row_maxima(out):
    for p in "ab":
        out["V_" + p] = out["Q_" + p].max(-1)
    return out


class WolfPHCLearner(_Learner):
    """Policy hill-climbers for both players (PHC and WoLF-PHC, Bowling & Veloso 2002) on a two-player auto-reset
    SoccerBatch: the Q-learners' two tables plus a mixed policy pi_p[nS, 5] and its running average avg_p per player on
    the device, the batch's lanes as actors (include/soccer_hip.h, "learners, policy hill-climbing").  run() enqueues
    and returns; read() and the properties synchronise and copy."""
    _C = "soccer_wolf_phc"
    _STATE = _lib.WolfPHCState
    _FIELDS = _WOLF_TABLES + (("visits", (_S, 25), np.uint64), ("updates", (_S,), np.uint64), ("alpha", None, C.c_double),
                              ("dscale", None, C.c_double), ("steps", None, C.c_uint64))
    _WHICH = _WOLF_WHICH

    def __init__(self, batch, discount_factor, **params):
        cfg, keep = wolf_phc_config(batch.nS, discount_factor, **params)
        self._create(batch, cfg)
        del keep                                   # (create has copied the fixed policies)
        self.discount_factor = float(discount_factor)

    def update(self, obs, act_a, act_b, reward, terminated, next_obs):
        """One learner step's reduce / update / policy step on a batch of transitions (reward is player A's): DeviceArrays
        (or device tensors) of one length, or numpy arrays, which are copied to the device first."""
        return self._update(obs, act_a, act_b, reward, terminated, next_obs)

    def read(self):
        """dict: Q_a / Q_b, pi_a / pi_b, avg_a / avg_b [nS, 5], V_a / V_b [nS] (the row maxima, computed here), visits[nS, 25],
        updates[nS], alpha, dscale, steps.  The policies plug into rollout(mixed_policies=...) and planners.exploitability
        as they are.  Synchronises."""
        return _row_maxima(self._read())

    alpha, dscale, steps = _field("alpha"), _field("dscale"), _field("steps")

    def exploitability(self, which="pi", theta=1e-10):
        """How badly the best possible opponent beats the pair of policies (which='pi') or of average policies
        (which='avg') the learners hold now, at their discount: planners.exploitability.  Synchronises and copies."""
        return self._exploitability(which, theta)

    def load(self, Q_a, Q_b, pi_a=None, pi_b=None, avg_a=None, avg_b=None, visits=None, updates=None, alpha=None, dscale=None,
             steps=None):
        """Resume from a checkpoint: everything derived is recomputed on the device.  With all of read()'s arrays and
        scalars a fresh learner continues bit for bit.  A policy array that is None is left as it is (those of a player
        that does not learn are ignored); without `visits` / `updates` the counts are zeroed."""
        assert Q_a is not None and Q_b is not None, "Q_a / Q_b are required"
        return self._load(dict(Q_a=Q_a, Q_b=Q_b, pi_a=pi_a, pi_b=pi_b, avg_a=avg_a, avg_b=avg_b, visits=visits, updates=updates,
                               alpha=alpha, dscale=dscale, steps=steps))


class WolfPopulation(_population_with_a_choice("pi")):
    """A population of policy hill-climbers (PHC / WoLF-PHC) on a two-player auto-reset SoccerBatch, a learner per lane:
    member i has its own Q_a, Q_b, pi_a, pi_b, avg_a, avg_b [nS, 5], updates[nS], alpha and dscale and learns from lane i alone
    (include/soccer_hip.h, "learners, a population of policy hill-climbers").  A fixed player's policy is per member.  run()
    enqueues and returns; read() and the properties synchronise and copy.  read(), load() and exploitability() take a range
    of members.  The evaluations take which='pi', the pair of policies, or which='avg', the pair of average policies."""
    _C = "soccer_wolf_population"
    _STATE = _lib.WolfPopulationState
    _FIELDS = _WOLF_TABLES + (("updates", (_S,), np.uint64), ("alpha", (), np.float64), ("dscale", (), np.float64),
                              ("steps", None, C.c_uint64))
    _WHICH = _WOLF_WHICH

    def __init__(self, batch, discount_factor, **params):
        cfg, keep = wolf_population_config(batch.n, batch.nS, discount_factor, **params)
        self._create(batch, cfg, keep[1])
        del keep                                   # (create has copied the parameters and the fixed policies)
        self.modes = (cfg.act_a, cfg.act_b)

    def read(self, first=0, count=None):
        """dict for members first .. first + count - 1 (count None: to the end): Q_a / Q_b, pi_a / pi_b, avg_a / avg_b
        [count, nS, 5], V_a / V_b [count, nS] (the row maxima, computed here), updates[count, nS], alpha[count],
        dscale[count], steps.  Synchronises."""
        return _row_maxima(self._read(None, first, count))

    alpha, steps = _field("alpha", "every member's learning rate, [n]"), _field("steps")
    dscale = _field("dscale", "every member's factor on both deltas, [n]")

    def load(self, Q_a=None, Q_b=None, pi_a=None, pi_b=None, avg_a=None, avg_b=None, updates=None, alpha=None, dscale=None, steps=None,
             first=0):
        """Resume members first .. first + count - 1 from a checkpoint (count is what the arrays hold; None = unchanged): the
        six tables [count, nS, 5], updates[count, nS], alpha[count] and dscale[count], steps for the population.  With what
        read() gave, a fresh population continues bit for bit.  A refused load changes nothing."""
        return self._load(dict(Q_a=Q_a, Q_b=Q_b, pi_a=pi_a, pi_b=pi_b, avg_a=avg_a, avg_b=avg_b, updates=updates, alpha=alpha,
                               dscale=dscale, steps=steps), first)

    def adopt(self, player, src, src_player, which="pi"):
        """Freeze: every member's fixed policy of `player` (0 = A, 1 = B) becomes the pi (which='pi') or avg (which='avg') of
        `src_player` of the same member of the population `src` on this batch, on the device, enqueued."""
        self._pair(which)
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


class MinimaxQPopulation(_Population):
    """A population of minimax-Q learners (Littman 1994) on a two-player auto-reset SoccerBatch, a learner per lane: member i
    has its own Q[nS, 5, 5], V[nS], pi_a / pi_b [nS, 5] and alpha and learns from lane i alone (include/soccer_hip.h, "learners,
    a population of minimax-Q learners").  run() enqueues and returns; read() and the properties synchronise and copy.  Whole
    populations run to gigabytes, so read(), load() and exploitability() take a range of members."""
    _C = "soccer_minimax_q_population"
    _FIELDS = (("Q", (_S, 5, 5), np.float64), ("V", (_S,), np.float64), ("pi_a", _ROWS, np.float64), ("pi_b", _ROWS, np.float64),
               ("alpha", (), np.float64), ("steps", None, C.c_uint64))

    def __init__(self, batch, discount_factor, **params):
        cfg, keep = minimax_q_population_config(batch.n, batch.nS, discount_factor, **params)
        self._create(batch, cfg, keep[1])
        del keep                                   # (create has copied the parameters and the fixed policies' thresholds)
        self.opponent = cfg.opponent

    def read(self, first=0, count=None):
        """dict for members first .. first + count - 1 (count None: to the end): Q[count, nS, 5, 5], V[count, nS], pi_a / pi_b
        [count, nS, 5], alpha[count], steps.  Synchronises."""
        return self._read(None, first, count)

    alpha, steps = _field("alpha", "every member's learning rate, [n]"), _field("steps")

    def load(self, Q=None, V=None, pi_a=None, pi_b=None, alpha=None, steps=None, first=0):
        """Resume members first .. first + count - 1 from a checkpoint (count is what the arrays hold; None = unchanged):
        Q[count, nS, 5, 5] and V[count, nS] in [-1, 1], pi_a / pi_b [count, nS, 5], alpha[count], steps for the population.  Q
        alone: V and the strategies of every live state of the range are re-solved on the device.  With V, pi_a and pi_b
        they are stored as given, so with what read() gave a fresh population continues bit for bit.  A refused load changes
        nothing."""
        return self._load(dict(Q=Q, V=V, pi_a=pi_a, pi_b=pi_b, alpha=alpha, steps=steps), first)


def _ordered_sum(x):
    """(((((0.0 + x[..., 0]) + x[..., 1]) + ...) + x[..., 4]): the device's order"""
    tot = np.zeros(x.shape[:-1])
    for k in range(5):
        tot = tot + x[..., k]
    return tot


def regret_policy(R):
    """policy(p, s) of a LEARN player by the definition's expression (include/soccer_hip.h, "learners, a population of regret
    matchers"), operation for operation, so it equals the device's: regrets [..., 5] -> the normalised positive part, 0.2
    where no regret is positive."""
    R = np.asarray(R, np.float64)
    pos = np.where(R > 0.0, R, 0.0)
    tot = _ordered_sum(pos)[..., None]
    return np.where(tot > 0.0, pos / np.where(tot > 0.0, tot, 1.0), 0.2)


def regret_average(Z):
    """The average policy of a LEARN player: policy sums [..., 5] -> Z / (the sum of the row, in the device's order), 0.2 where
    that sum is 0."""
    Z = np.asarray(Z, np.float64)
    tot = _ordered_sum(Z)[..., None]
    return np.where(tot == 0.0, 0.2, Z / np.where(tot == 0.0, 1.0, tot))


class RegretPopulation(_population_with_a_choice("avg")):
    """A population of regret matchers (Hart & Mas-Colell 2000; per state, with Q-values for counterfactual values) on a
    two-player auto-reset SoccerBatch, a learner per lane: member i has its own Q_a, Q_b, cumulative regrets R_a, R_b and
    policy sums Z_a, Z_b [nS, 5], updates[nS] and alpha and learns from lane i alone (include/soccer_hip.h, "learners, a
    population of regret matchers").  plus floors the regrets at 0 (regret matching+), linear weighs a step's policy by the
    state's visit count.  A fixed player's policy is shared or per member.  run() enqueues and returns; read() and the
    properties synchronise and copy.  read(), load() and the evaluations take a range of members.  The evaluations take
    which='avg', the pair of average policies (the one that carries the no-regret guarantee), or which='pi', the pair of
    current policies."""
    _C = "soccer_regret_population"
    _STATE = _lib.RegretPopulationState
    _FIELDS = tuple((k, _ROWS, np.float64) for k in ("Q_a", "Q_b", "R_a", "R_b", "Z_a", "Z_b")) + (
        ("updates", (_S,), np.uint64), ("alpha", (), np.float64), ("steps", None, C.c_uint64))
    _WHICH = {"avg": ("avg_a", "avg_b"), "pi": ("pi_a", "pi_b")}

    def __init__(self, batch, discount_factor, **params):
        cfg, keep = regret_population_config(batch.n, batch.nS, discount_factor, **params)
        self._create(batch, cfg, keep[1])
        self.modes = (cfg.act_a, cfg.act_b)
        self.plus, self.linear = bool(cfg.plus), bool(cfg.linear)
        # a fixed player's rows, [nS, 5] or [n, nS, 5]: read() hands them back (create has copied them to the device)
        self._fixed = [None if x is None and y is None else (x if y is None else y).copy() for x, y in zip(*keep[0])]
        del keep

    def _policies(self, first, count, keys):
        return self.read(first, count)

    def read(self, first=0, count=None):
        """dict for members first .. first + count - 1 (count None: to the end): Q_a / Q_b, R_a / R_b, Z_a / Z_b [count, nS, 5],
        updates[count, nS], alpha[count], steps; and, computed here by the definition's expressions, pi_a / pi_b (the current
        policies) and avg_a / avg_b (the average policies) [count, nS, 5]; a fixed or uniform player reads back its own rows
        for both.  Synchronises."""
        first, count = self._range(first, count)
        out = self._read(None, first, count)
        for p, name in enumerate("ab"):
            if self.modes[p] == _lib.PHC_LEARN:
                out["pi_" + name], out["avg_" + name] = regret_policy(out["R_" + name]), regret_average(out["Z_" + name])
                continue
            fixed = self._fixed[p]
            rows = np.full((count, self.nS, 5), 0.2) if fixed is None else (
                np.broadcast_to(fixed, (count, self.nS, 5)).copy() if fixed.ndim == 2 else fixed[first:first + count].copy())
            out["pi_" + name], out["avg_" + name] = rows, rows.copy()
        return out

    alpha, steps = _field("alpha", "every member's learning rate, [n]"), _field("steps")

    def load(self, Q_a=None, Q_b=None, R_a=None, R_b=None, Z_a=None, Z_b=None, updates=None, alpha=None, steps=None, first=0):
        """Resume members first .. first + count - 1 from a checkpoint (count is what the arrays hold; None = unchanged): the
        six tables [count, nS, 5] — Q in [-1, 1], R finite (and >= 0 under plus), Z finite and >= 0; those of a player that
        does not learn are ignored —, updates[count, nS], alpha[count], steps for the population.  With what read() gave, a
        fresh population continues bit for bit.  A refused load changes nothing."""
        for k, x, nonneg in (("R_a", R_a, self.plus), ("R_b", R_b, self.plus), ("Z_a", Z_a, True), ("Z_b", Z_b, True)):
            if x is not None:
                x = np.asarray(x, np.float64)
                assert np.isfinite(x).all() and (not nonneg or (x >= 0.0).all()), "%s must be finite%s" % (k, " and >= 0" if nonneg else "")
        return self._load(dict(Q_a=Q_a, Q_b=Q_b, R_a=R_a, R_b=R_b, Z_a=Z_a, Z_b=Z_b, updates=updates, alpha=alpha, steps=steps), first)


class RegretLearner(_Learner):
    """Regret matchers for both players with ONE table that every lane feeds (the shared form of RegretPopulation) on a
    two-player auto-reset SoccerBatch: Q_a, Q_b, the cumulative regrets R_a, R_b and the policy sums Z_a, Z_b [nS, 5] on the
    device, the batch's lanes as actors (include/soccer_hip.h, "learners, regret matching").  plus floors the regrets at 0
    (regret matching+), linear weighs a step's policy by the state's update count.  run() enqueues and returns; read() and
    the properties synchronise and copy.  exploitability takes which='avg', the pair of average policies (the one that
    carries the no-regret guarantee), or which='pi', the pair of current policies."""
    _C = "soccer_regret_learner"
    _STATE = _lib.RegretLearnerState
    _FIELDS = tuple((k, _ROWS, np.float64) for k in ("Q_a", "Q_b", "R_a", "R_b", "Z_a", "Z_b")) + (
        ("visits", (_S, 25), np.uint64), ("updates", (_S,), np.uint64), ("alpha", None, C.c_double), ("steps", None, C.c_uint64))
    _WHICH = {"avg": ("avg_a", "avg_b"), "pi": ("pi_a", "pi_b")}

    def __init__(self, batch, discount_factor, **params):
        cfg, keep = regret_learner_config(batch.nS, discount_factor, **params)
        self._create(batch, cfg)
        self.discount_factor = float(discount_factor)
        self.modes = (cfg.act_a, cfg.act_b)
        self.plus, self.linear = bool(cfg.plus), bool(cfg.linear)
        # a fixed player's rows [nS, 5]: read() hands them back (create has copied them to the device)
        self._fixed = [None if x is None else x.copy() for x in keep]
        del keep

    def update(self, obs, act_a, act_b, reward, terminated, next_obs):
        """One learner step's reduce / update / regret step on a batch of transitions (reward is player A's): DeviceArrays
        (or device tensors) of one length, or numpy arrays, which are copied to the device first."""
        return self._update(obs, act_a, act_b, reward, terminated, next_obs)

    def read(self):
        """dict: Q_a / Q_b, R_a / R_b, Z_a / Z_b [nS, 5], visits[nS, 25], updates[nS], alpha, steps; and, computed here by the
        definition's expressions, pi_a / pi_b (the current policies) and avg_a / avg_b (the average policies) [nS, 5]; a fixed
        or uniform player reads back its own rows for both.  Synchronises."""
        out = self._read()
        for p, name in enumerate("ab"):
            if self.modes[p] == _lib.PHC_LEARN:
                out["pi_" + name], out["avg_" + name] = regret_policy(out["R_" + name]), regret_average(out["Z_" + name])
                continue
            rows = np.full((self.nS, 5), 0.2) if self._fixed[p] is None else self._fixed[p].copy()
            out["pi_" + name], out["avg_" + name] = rows, rows.copy()
        return out

    alpha, steps = _field("alpha"), _field("steps")

    def exploitability(self, which="avg", theta=1e-10):
        """How badly the best possible opponent beats the pair of average policies (which='avg') or of current policies
        (which='pi') the learners hold now, at their discount: planners.exploitability.  Synchronises and copies."""
        return self._exploitability(which, theta)

    def load(self, Q_a, Q_b, R_a=None, R_b=None, Z_a=None, Z_b=None, visits=None, updates=None, alpha=None, steps=None):
        """Resume from a checkpoint: everything derived is recomputed on the device.  Q in [-1, 1], R finite (and >= 0 under
        plus), Z finite and >= 0.  With all of read()'s arrays and scalars a fresh learner continues bit for bit.  A regret or
        policy-sum array that is None is left as it is (those of a player that does not learn are ignored); without `visits`
        / `updates` the counts are zeroed.  A refused load changes nothing."""
        assert Q_a is not None and Q_b is not None, "Q_a / Q_b are required"
        return self._load(dict(Q_a=Q_a, Q_b=Q_b, R_a=R_a, R_b=R_b, Z_a=Z_a, Z_b=Z_b, visits=visits, updates=updates, alpha=alpha,
                               steps=steps))


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
        b._checked(code, tr)
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
