"""The four population wrappers driven against a stand-in batch: no library, no GPU.  The stand-in's library answers create /
run / destroy with 0, writes values that identify the member and the field into every output a read hands it, and records
every call; its best_response and pair evaluators record what they get and return values that identify the policies and the
discount.  So the host code of the wrappers (ranges, chunks of 256, grouping by discount, which policy pair goes where,
load's checks and the C argument order) is held to what it does, whatever shape it is written in."""
import ctypes as C

import numpy as np
import pytest

from gym_soccer_littman94_amd import _lib
from gym_soccer_littman94_amd.core import MinimaxQPopulation, OpponentModelPopulation, QPopulation, WolfPopulation

N, NS, STEPS = 300, 6, 7
F8, U8 = np.float64, np.uint64
# members' discounts: both chunks of 256 hold both values, and ranges with one discount exist
GAMMA = np.where((np.arange(N) // 100 == 1) | (np.arange(N) >= 280), 0.5, 0.9)

# the fields of each kind's read / load in the C argument order (include/soccer_hip.h): key, shape after [count], dtype
ABI = {
    "soccer_q_population": (False, [("Q_a", (NS, 5), F8), ("Q_b", (NS, 5), F8), ("alpha", (), F8)]),
    "soccer_om_population": (False, [("Q_a", (NS, 5, 5), F8), ("Q_b", (NS, 5, 5), F8), ("C_a", (NS, 5), U8), ("C_b", (NS, 5), U8),
                                     ("alpha", (), F8)]),
    "soccer_minimax_q_population": (False, [("Q", (NS, 5, 5), F8), ("V", (NS,), F8), ("pi_a", (NS, 5), F8), ("pi_b", (NS, 5), F8),
                                            ("alpha", (), F8)]),
    "soccer_wolf_population": (True, [("Q_a", (NS, 5), F8), ("Q_b", (NS, 5), F8), ("pi_a", (NS, 5), F8), ("pi_b", (NS, 5), F8),
                                      ("avg_a", (NS, 5), F8), ("avg_b", (NS, 5), F8), ("updates", (NS,), U8), ("alpha", (), F8),
                                      ("dscale", (), F8)]),
}


def pattern(members, field, shape):
    """What the stand-in writes for `members` into field number `field`.  Tables with a last axis of 5 are one-hot rows that
    spell the member in base 5 over states 0 .. 3 and the field over states 4 and 5, so that an argmax, a row maximum or a
    frequency of them still names both; [nS] arrays hold the member, per-member scalars member / 1024."""
    m = np.asarray(members)
    if shape == ():
        return m / 1024.0
    if shape == (NS,):
        return np.repeat(m[:, None], NS, 1)
    digits = np.stack([m // 5 ** s % 5 for s in range(4)] + [np.full(m.shape, field % 5), np.full(m.shape, field // 5)], 1)
    rows = np.eye(5)[digits]                                            # [count, nS, 5]
    return rows if len(shape) == 2 else np.repeat(rows[..., None], 5, 3)    # [.., own action, the other's]: the same for each


def decode(policies):
    """(members, fields) of [P, nS, 5] policies derived from pattern()'s tables"""
    d = np.asarray(policies).argmax(2)
    return sum(d[:, s] * 5 ** s for s in range(4)), d[:, 4] + 5 * d[:, 5]


class Library:
    """libsoccer_hip.so's learner entry points, as far as the wrappers use them"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            assert len(args) == len(_lib.PROTOTYPES[name][1]), name
            if name.endswith("_read") and "league" not in name:
                self.read(name[:-5], *args[2:])
            return 0
        return call

    def outputs(self, kind, args):
        """[(field number, key, shape, dtype, address or None)], the steps argument"""
        struct, fields = ABI[kind]
        if struct:
            state = args[0]._obj
            assert [n for n, _ in state._fields_] == [k for k, _, _ in fields] + ["steps"]
            return [(f, k, s, dt, getattr(state, k)) for f, (k, s, dt) in enumerate(fields)], state.steps
        assert len(args) == len(fields) + 1
        return [(f, k, s, dt, p) for (f, (k, s, dt)), p in zip(enumerate(fields), args)], args[-1]

    def read(self, kind, first, count, *args):
        outs, steps = self.outputs(kind, args)
        for f, _, shape, dt, p in outs:
            if p and count:
                size = count * int(np.prod(shape, dtype=np.int64))
                np.ctypeslib.as_array((C.c_uint64 * size).from_address(p)).view(dt).reshape((count,) + shape)[...] = \
                    pattern(np.arange(first, first + count), f, shape)
        if steps:
            (steps.contents if ABI[kind][0] else steps._obj).value = STEPS


class Batch:
    """What the wrappers use of a SoccerBatch"""

    def __init__(self):
        self.lib, self.h, self.n, self.nS, self._learners, self.calls = Library(), C.c_void_p(1), N, NS, set(), []

    def _check(self, code):
        assert code == 0

    def best_response(self, policy, player, theta, discount_factor, max_sweeps=1000000):
        members, fields = decode(policy)
        self.calls.append(("best_response", members, fields, player, discount_factor))
        V = np.repeat((members + 1000 * fields + discount_factor)[:, None], NS, 1)
        return None, V, None, None

    def _pair(self, what, pi_a, pi_b, discount, **more):
        self.calls.append((what, decode(pi_a), decode(pi_b), discount, more))
        return decode(pi_a)[0][:, None] * 1000.0 - decode(pi_b)[0][None, :] + discount

    def cross_play(self, pi_a, pi_b, theta, discount_factor):
        return self._pair("cross_play", pi_a, pi_b, discount_factor), "iterations"

    def match_outcomes(self, pi_a, pi_b, theta, continue_prob):
        return {"match_outcomes": self._pair("match_outcomes", pi_a, pi_b, continue_prob)}

    def occupancy(self, pi_a, pi_b, theta, continue_prob, features=None, values=False):
        return {"occupancy": self._pair("occupancy", pi_a, pi_b, continue_prob, features=features, values=values)}

    def solve_meta_game(self, payoff, max_pivots=None):
        self.calls.append(("solve_meta_game", payoff, max_pivots))
        return {"x": "x", "y": "y", "value": 0.5, "lo": 0.25, "hi": 0.75, "status": 1, "pivots": 3}


# the wrapper, its C prefix, `which`, and the fields behind player A's and player B's policies of that choice
CASES = [(QPopulation, "soccer_q_population", None, 0, 1),                      # the greedy policies of Q_a and Q_b
         (OpponentModelPopulation, "soccer_om_population", "greedy", 0, 1),     # the greedy answers of Q_a and Q_b
         (OpponentModelPopulation, "soccer_om_population", "model", 3, 2),      # model_a is C_b as frequencies, model_b C_a
         (WolfPopulation, "soccer_wolf_population", "pi", 2, 3),
         (WolfPopulation, "soccer_wolf_population", "avg", 4, 5),
         (MinimaxQPopulation, "soccer_minimax_q_population", None, 2, 3)]
IDS = ["q", "om-greedy", "om-model", "wolf-pi", "wolf-avg", "minimax-q"]
KINDS = [c for c in CASES if c[2] in (None, "greedy", "pi")]
KIND_IDS = ["q", "om", "wolf", "minimax-q"]


def make(cls):
    batch = Batch()
    pop = cls(batch, GAMMA)
    assert [c[0].rpartition("_")[2] for c in batch.lib.calls] == ["create"] and pop in batch._learners
    assert np.array_equal(pop.discount_factor, GAMMA)
    del batch.lib.calls[:]
    return batch, pop


@pytest.mark.parametrize("cls, kind, which, fa, fb", CASES, ids=IDS)
def test_exploitability_solves_chunks_of_one_discount(cls, kind, which, fa, fb):
    batch, pop = make(cls)
    first, count = 3, 295                                              # members 3 .. 297: chunks 3 .. 258 and 259 .. 297
    out = pop.exploitability(first=first, count=count, **({"which": which} if which else {}))
    members = np.arange(first, first + count)
    for key, field in (("v_a", fa), ("v_b", fb)):
        assert np.array_equal(out[key], np.repeat((members + 1000 * field + GAMMA[members])[:, None], NS, 1))
    assert np.array_equal(out["gap"], out["v_b"] - out["v_a"]) and sorted(out) == ["gap", "v_a", "v_b"]
    seen = {0: [], 1: []}
    for what, m, f, player, g in batch.calls:
        assert what == "best_response" and 1 <= m.size <= _lib.BR_MAX_POLICIES
        assert (GAMMA[m] == g).all() and (f == (fa, fb)[player]).all()   # one discount, the members', and the player's own key
        seen[player].append(m)
    assert np.array_equal(np.sort(np.concatenate(seen[0])), members) and np.array_equal(np.sort(np.concatenate(seen[1])), members)
    assert len(batch.calls) == 8                                        # two chunks x two discounts x two players


@pytest.mark.parametrize("cls, kind, which, fa, fb", CASES, ids=IDS)
@pytest.mark.parametrize("method, name", [("cross_play", "discount_factor"), ("match_outcomes", "continue_prob"),
                                          ("occupancy", "continue_prob")])
def test_pair_evaluators_get_the_range_in_order_and_its_discount(cls, kind, which, fa, fb, method, name):
    batch, pop = make(cls)
    w = {"which": which} if which else {}
    run = getattr(pop, method)
    extra = {"features": "F", "values": True} if method == "occupancy" else {}

    def result(r):
        return r[0] if method == "cross_play" else r[method]
    # a range across the chunk boundary with its discount given; one with a common discount; the evaluator's own extras
    for first, count, given, expect in ((10, 280, 0.7, 0.7), (200, 60, None, 0.9), (100, 1, None, 0.5)):
        del batch.calls[:]
        r = result(run(first=first, count=count, **{name: given}, **w, **extra))
        members = np.arange(first, first + count)
        (what, (ma, fa_), (mb, fb_), discount, more), = batch.calls
        assert what == method and discount == expect and isinstance(discount, float) and more == extra
        assert np.array_equal(ma, members) and np.array_equal(mb, members) and (fa_ == fa).all() and (fb_ == fb).all()
        assert np.array_equal(r, members[:, None] * 1000.0 - members[None, :] + expect)
    del batch.calls[:]
    with pytest.raises(ValueError, match=r"members 90 and 100 have different discounts \(0\.9 and 0\.5\): pass %s" % name):
        run(first=90, count=20, **w)
    for first, count in ((0, 0), (0, 1025), (290, 20), (301, None)):
        with pytest.raises(AssertionError):
            run(first=first, count=count, **{name: 0.9}, **w)
    if which:
        for bad in ("pi_a", "greedy " if which in ("pi", "avg") else "pi", None):
            with pytest.raises(AssertionError, match="which must be"):
                run(which=bad, first=0, count=4, **{name: 0.9})
            with pytest.raises(AssertionError, match="which must be"):
                pop.exploitability(which=bad)
    assert batch.calls == []


@pytest.mark.parametrize("cls, kind, which, fa, fb", CASES, ids=IDS)
def test_meta_game_is_cross_play_plus_the_solve(cls, kind, which, fa, fb):
    batch, pop = make(cls)
    out = pop.meta_game(first=20, count=5, max_pivots=11, **({"which": which} if which else {}))
    members = np.arange(20, 25)
    payoff = members[:, None] * 1000.0 - members[None, :] + 0.9
    assert [c[0] for c in batch.calls] == ["cross_play", "solve_meta_game"]
    assert np.array_equal(batch.calls[1][1], payoff) and batch.calls[1][2] == 11
    assert np.array_equal(out["payoff"], payoff) and out["iterations"] == "iterations"
    assert np.array_equal(out["row_min"], payoff.min(1)) and np.array_equal(out["col_max"], payoff.max(0))
    assert out["bounds"] == (payoff.min(1).max(), payoff.max(0).min()) and out["gain"] == 0.25 - out["bounds"][0]
    assert (out["x"], out["y"], out["value"], out["lo"], out["hi"], out["status"]) == ("x", "y", 0.5, 0.25, 0.75, 1)
    assert "pivots" not in out


@pytest.mark.parametrize("cls, kind, which, fa, fb", KINDS, ids=KIND_IDS)
def test_read_and_the_properties_come_from_the_c_argument_order(cls, kind, which, fa, fb):
    batch, pop = make(cls)
    first, count = 250, 12
    r = pop.read(first, count)
    for f, (key, shape, dt) in enumerate(ABI[kind][1]):
        assert r[key].dtype == dt and np.array_equal(r[key], pattern(np.arange(first, first + count), f, shape)), key
    assert r["steps"] == STEPS and pop.steps == STEPS
    assert pop.read(295)["alpha"].shape == (5,)                          # count None: to the end
    assert np.array_equal(pop.alpha, np.arange(N) / 1024.0)
    if cls is WolfPopulation:
        assert np.array_equal(pop.dscale, np.arange(N) / 1024.0)
    for bad in ((-1, 1), (0, N + 1), (N, 1)):
        with pytest.raises(AssertionError, match="outside the population"):
            pop.read(*bad)


@pytest.mark.parametrize("cls, kind, which, fa, fb", KINDS, ids=KIND_IDS)
def test_load_checks_first_and_hands_pointers_over_in_the_c_argument_order(cls, kind, which, fa, fb):
    batch, pop = make(cls)
    struct, fields = ABI[kind]
    good = {key: np.zeros((2,) + shape, dt) for key, shape, dt in fields}

    def loaded():
        """the positions of the non-NULL arguments of the one load that was recorded, and (first, count)"""
        (name, args), = batch.lib.calls
        del batch.lib.calls[:]
        assert name == kind + "_load"
        outs, steps = batch.lib.outputs(kind, args[4:])
        return [k for _, k, _, _, p in outs if p] + (["steps"] if steps else []), args[2:4]
    for key in good:
        assert pop.load(first=5, **{key: good[key]}) is pop
        assert loaded() == ([key], (5, 2))
    pop.load(steps=9)
    assert loaded() == (["steps"], (0, 0))
    pop.load(first=N - 2, steps=1, **good)
    assert loaded() == ([k for k, _, _ in fields] + ["steps"], (N - 2, 2))

    q = fields[0][0]                                                    # "Q_a" or "Q"
    one_off = np.zeros((2,) + fields[0][1]); one_off[1, 1] = 1.5        # a value outside [-1, 1] in a live state
    row_0 = np.zeros((2,) + fields[0][1]); row_0[:, 0] = 7.0            # row 0, the terminal observation, is not checked
    refused = [{key: np.zeros((2,) + shape[:-1] + (4,), dt)} for key, shape, dt in fields if shape] + \
              [{key: np.zeros((2, 2), dt)} for key, shape, dt in fields if not shape] + \
              [{q: one_off}, {q: -one_off}, {"alpha": np.array([0.5, 1.5])}, {"alpha": np.array([-0.5, 0.5])},
               {q: good[q], "alpha": np.zeros(3)}, {fields[1][0]: np.zeros((3,) + fields[1][1], fields[1][2]), q: good[q]},
               {"alpha": np.zeros(2), "first": N - 1}]
    for kw in refused:
        with pytest.raises(AssertionError):
            pop.load(**kw)
        assert batch.lib.calls == [], kw                                # refused before any library call
    pop.load(**{q: row_0})
    assert loaded() == ([q], (0, 2))
