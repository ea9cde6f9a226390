"""The RegretPopulation wrapper driven against the stand-in batch of tests/test_population_wrappers_host.py: no library, no
GPU.  The stand-in serves as it is with one more row in its ABI table, and its checks are called here on the new kind: the C
argument order of read and load, ranges, chunks of 256, grouping by discount, which pair of policies `which` sends.  Then what
is the kind's own: 'avg' is the default pair, every refusal of load, and the derived rows."""
import os
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd.core import RegretPopulation, regret_average, regret_policy

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_population_wrappers_host as host  # noqa: E402

N, NS, GAMMA, F8, U8 = host.N, host.NS, host.GAMMA, host.F8, host.U8
KIND = "soccer_regret_population"
# soccer_regret_population_state, in the C order (include/soccer_hip.h); steps follows
host.ABI[KIND] = (True, [("Q_a", (NS, 5), F8), ("Q_b", (NS, 5), F8), ("R_a", (NS, 5), F8), ("R_b", (NS, 5), F8), ("Z_a", (NS, 5), F8),
                         ("Z_b", (NS, 5), F8), ("updates", (NS,), U8), ("alpha", (), F8)])
# `which` and the fields behind player A's and player B's policies: avg from Z_a and Z_b, pi from R_a and R_b (the stand-in's
# tables are one-hot rows, which both derivations give back)
CASES = [(RegretPopulation, KIND, "avg", 4, 5), (RegretPopulation, KIND, "pi", 2, 3)]
IDS = ["regret-avg", "regret-pi"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exploitability_solves_chunks_of_one_discount(case):
    host.test_exploitability_solves_chunks_of_one_discount(*case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("method, name", [("cross_play", "discount_factor"), ("match_outcomes", "continue_prob"), ("occupancy", "continue_prob")])
def test_pair_evaluators_get_the_range_in_order_and_its_discount(case, method, name):
    host.test_pair_evaluators_get_the_range_in_order_and_its_discount(*case, method, name)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_meta_game_is_cross_play_plus_the_solve(case):
    host.test_meta_game_is_cross_play_plus_the_solve(*case)


def test_read_and_the_properties_come_from_the_c_argument_order():
    host.test_read_and_the_properties_come_from_the_c_argument_order(*CASES[0])


def test_load_checks_first_and_hands_pointers_over_in_the_c_argument_order():
    host.test_load_checks_first_and_hands_pointers_over_in_the_c_argument_order(*CASES[0])


def test_avg_is_the_default_pair():
    batch, pop = host.make(RegretPopulation)
    pop.exploitability(first=0, count=4)
    pop.cross_play(first=0, count=4, discount_factor=0.9)
    pop.match_outcomes(first=0, count=4, continue_prob=0.9)
    pop.occupancy(first=0, count=4, continue_prob=0.9)
    pop.meta_game(first=0, count=4, discount_factor=0.9)
    fields = []
    for c in batch.calls:
        if c[0] == "best_response":
            fields.append((c[3], set(c[2].tolist())))
        elif c[0] != "solve_meta_game":
            fields.append((0, set(c[1][1].tolist()))); fields.append((1, set(c[2][1].tolist())))
    assert fields and all(f == {(4, 5)[player]} for player, f in fields)              # Z_a and Z_b


@pytest.mark.parametrize("plus", [True, False], ids=["plus", "plain"])
def test_every_refusal_of_load_comes_before_any_library_call(plus):
    batch = host.Batch()
    pop = RegretPopulation(batch, GAMMA, plus=plus)
    del batch.lib.calls[:]
    rows = np.zeros((2, NS, 5))

    def bad(value, row=1):
        x = rows.copy(); x[1, row, 3] = value
        return x
    refused = [dict(Z_a=bad(-1e-9)), dict(Z_b=bad(float("nan"))), dict(Z_a=bad(float("inf"))), dict(R_a=bad(float("nan"))),
               dict(R_b=bad(float("-inf"))), dict(Q_a=bad(1.5)), dict(Q_b=bad(-1.0000001)), dict(alpha=np.array([0.5, 1.5])),
               dict(R_a=np.zeros((2, NS, 4))), dict(Z_b=np.zeros((2, NS + 1, 5))), dict(updates=np.zeros((2, NS + 1), np.uint64)),
               dict(R_a=rows, Z_a=np.zeros((3, NS, 5))), dict(Q_a=rows, first=N - 1), dict(Q_a=rows, first=-1)]
    if plus:
        refused += [dict(R_a=bad(-0.5)), dict(R_b=bad(-1e-300))]
    for kw in refused:
        with pytest.raises(AssertionError):
            pop.load(**kw)
        assert batch.lib.calls == [], kw
    if not plus:                                                        # without plus a negative regret is a regret
        pop.load(R_a=bad(-0.5), R_b=bad(-1e-300))
        (name, args), = batch.lib.calls
        assert name == KIND + "_load" and args[2:4] == (0, 2)
        del batch.lib.calls[:]
    pop.load(Q_a=bad(7.0, row=0))                                       # row 0, the terminal observation, is not checked
    assert len(batch.lib.calls) == 1


def test_the_derived_rows():
    members = np.arange(250, 262)
    batch, pop = host.make(RegretPopulation)
    r = pop.read(250, 12)
    assert sorted(r) == sorted(["Q_a", "Q_b", "R_a", "R_b", "Z_a", "Z_b", "updates", "alpha", "steps", "pi_a", "pi_b", "avg_a", "avg_b"])
    for name, f in (("pi_a", 2), ("pi_b", 3), ("avg_a", 4), ("avg_b", 5)):                 # one-hot rows derive to themselves
        assert np.array_equal(r[name], host.pattern(members, f, (NS, 5))), name
    # the expressions, on rows that are not one-hot: the ordered sum, the fallback
    R = np.array([[0.1, -0.2, 0.3, 0.0, 0.7], [-1.0, 0.0, -0.0, -2.0, -3.0]])
    tot = (((0.0 + 0.1) + 0.0) + 0.3 + 0.0) + 0.7
    assert regret_policy(R).tolist() == [[0.1 / tot, 0.0, 0.3 / tot, 0.0, 0.7 / tot], [0.2] * 5]
    Z = np.array([[0.1, 0.2, 0.3, 0.0, 0.7], [0.0] * 5])
    tot = (((0.0 + 0.1) + 0.2) + 0.3 + 0.0) + 0.7
    assert regret_average(Z).tolist() == [[0.1 / tot, 0.2 / tot, 0.3 / tot, 0.0, 0.7 / tot], [0.2] * 5]
    # a fixed or uniform player reads back its own rows for both: shared, per member (the range's slice), uniform
    rng = np.random.default_rng(3)
    shared, each = rng.dirichlet(np.ones(5), NS), rng.dirichlet(np.ones(5), (N, NS))
    for kw, want_a, want_b in ((dict(act_a=shared, act_b="learn"), np.broadcast_to(shared, (12, NS, 5)), host.pattern(members, 3, (NS, 5))),
                               (dict(act_a="learn", act_b=each), host.pattern(members, 2, (NS, 5)), each[250:262]),
                               (dict(act_a="uniform", act_b="uniform"), np.full((12, NS, 5), 0.2), np.full((12, NS, 5), 0.2))):
        pop = RegretPopulation(host.Batch(), GAMMA, **kw)
        r = pop.read(250, 12)
        assert np.array_equal(r["pi_a"], want_a) and np.array_equal(r["pi_b"], want_b)
        if not isinstance(kw["act_a"], str) or kw["act_a"] == "uniform":
            assert np.array_equal(r["avg_a"], want_a)
        if not isinstance(kw["act_b"], str) or kw["act_b"] == "uniform":
            assert np.array_equal(r["avg_b"], want_b)


def test_the_config_carries_the_flags_and_the_policies():
    from gym_soccer_littman94_amd import _lib
    from gym_soccer_littman94_amd.core import regret_population_config
    cfg, ((shared, each), arrays) = regret_population_config(8, NS, 0.9)
    assert (cfg.plus, cfg.linear, cfg.act_a, cfg.act_b) == (1, 0, _lib.PHC_LEARN, _lib.PHC_LEARN)
    assert not any((cfg.policy_a, cfg.policy_b, cfg.policy_a_per_member, cfg.policy_b_per_member, cfg.alpha_per_member))
    pol, per = np.full((NS, 5), 0.2), np.full((8, NS, 5), 0.2)
    cfg, ((shared, each), arrays) = regret_population_config(8, NS, np.linspace(0.1, 0.9, 8), plus=False, linear=True, act_a=pol, act_b=per)
    assert (cfg.plus, cfg.linear, cfg.act_a, cfg.act_b) == (0, 1, _lib.PHC_FIXED, _lib.PHC_FIXED)
    assert cfg.policy_a == shared[0].ctypes.data and cfg.policy_b_per_member == each[1].ctypes.data and not cfg.policy_b and not cfg.policy_a_per_member
    assert cfg.discount_factor_per_member == arrays["discount_factor"].ctypes.data
    for kw, msg in ((dict(plus=2), "plus"), (dict(linear="yes"), "linear"), (dict(act_a="greedy"), "act_a"), (dict(explor=1.5), "explor"),
                    (dict(act_b=np.full((NS, 5), 0.3)), "fixed act_b"), (dict(alpha=np.full(9, 0.5)), "one value per lane")):
        with pytest.raises(AssertionError, match=msg):
            regret_population_config(8, NS, 0.9, **kw)
