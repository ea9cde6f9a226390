"""The vectorised numpy restatement of the population of regret matchers (tests/regret_population_np.py) is n separate
one-member instances bit for bit, does what the definition says on a hand case, keeps its invariants (no negative regret and no
-0.0 under plus, the visit counts add up to the learned transitions), takes every branch in the short runs the GPU tests use,
and learns: against a uniform player B the members' average policy of player A beats what a uniform A scores, exactly
evaluated (tests/best_response_np.py).  tests/test_gpu_regret_population.py pins the device to this restatement bit for bit,
so this guards the yardstick where there is no GPU."""
import os
import sys
import time

import numpy as np
import pytest

from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_response_np as br  # noqa: E402
from cross_play_np import isd_obs, kickoff  # noqa: E402
from minimax_q_np import shapley_lists  # noqa: E402
from q_population_np import QPopulationNumpy  # noqa: E402
from regret_population_np import ROWS, RegretPopulationNumpy, assert_regret_population_equal, average, ordered_sum, policy  # noqa: E402

GAMMA = 0.9

# ---- the short runs tests/test_gpu_regret_population.py repeats on the device ------------------------------------------------
T_RUN, SEED = 60, 1994
RUN_KW = dict(explor=0.2, decay=0.99, alpha=0.9)
# width, height, slip, act_a, act_b, members, max_steps, plus, linear.  Member counts: a single lane, a few lanes, a ragged
# wave, a ragged workgroup.  Every case starts from a loaded state (RegretPopulationNumpy.load).  'shared': one fixed policy
# for every member; 'each': a fixed policy per member.  max_steps = 5: episodes truncate.
RUN_CASES = [(5, 4, 0.0, "learn", "uniform", 1, 100, True, False),
             (5, 4, 0.0, "learn", "learn", 3, 100, False, False),
             (5, 4, 0.2, "learn", "learn", 67, 100, True, True),
             (5, 4, 0.2, "learn", "learn", 259, 5, False, True),
             (7, 5, 0.3, "shared", "learn", 67, 100, True, False),
             (5, 4, 0.0, "learn", "each", 259, 5, True, False)]
RUN_IDS = ["5x4 slip 0 learn-uniform 1 plus", "5x4 slip 0 learn-learn 3 plain", "5x4 slip 0.2 learn-learn 67 plus linear",
           "5x4 slip 0.2 learn-learn 259 linear truncating", "7x5 slip 0.3 fixed shared-learn 67 plus",
           "5x4 slip 0 learn-fixed per member 259 plus truncating"]


def act(name, n, nS):
    """'shared': one fixed policy; 'each': a fixed policy per member"""
    if isinstance(name, str) and name == "shared":
        return np.random.default_rng(12).dirichlet(np.ones(5), nS)
    if isinstance(name, str) and name == "each":
        return np.random.default_rng(11).dirichlet(np.ones(5), (n, nS))
    return name


_REFERENCE = {}


def reference_run(w, h, slip, act_a, act_b, n, max_steps=100, plus=True, linear=False, T=T_RUN, seed=SEED):
    """(oracle, restatement, the loaded state it started from) after T steps; computed once per case and left unchanged"""
    key = (w, h, slip, act_a, act_b, n, max_steps, plus, linear, T, seed)
    if key not in _REFERENCE:
        o = Oracle(w, h, slip, n=n, seed=seed, autoreset=True, max_steps=max_steps)
        ref = RegretPopulationNumpy(n, o.nS, GAMMA, plus=plus, linear=linear, act_a=act(act_a, n, o.nS), act_b=act(act_b, n, o.nS), **RUN_KW)
        start = ref.load(np.random.default_rng(seed + n))
        ref.run(o, o.reset(), T)
        _REFERENCE[key] = (o, ref, start)
    return _REFERENCE[key]


def test_it_subclasses_the_q_population_s_restatement():
    assert issubclass(RegretPopulationNumpy, QPopulationNumpy)


@pytest.mark.parametrize("case", RUN_CASES, ids=RUN_IDS)
def test_the_short_runs_take_every_branch(case):
    w, h, slip, act_a, act_b, n, max_steps, plus, linear = case
    o, ref, start = reference_run(*case)
    print("%dx%d slip %g (%s, %s), %d members, plus %d linear %d: uniform fallback %d, floor %d; s' == s %d, terminated %d, truncated "
          "only %d" % (w, h, slip, act_a, act_b, n, plus, linear, ref.n_uniform, ref.n_floor, ref.n_same, ref.n_terminated,
                       ref.n_truncated_only))
    assert ref.n_left_out == 0 and ref.steps == T_RUN and ref.n_learned == n * T_RUN
    assert ref.n_uniform > 0                                        # a loaded row with no positive regret was met
    assert (ref.n_floor > 0) == plus
    if n > 3:
        assert ref.n_same > 0 and ref.n_terminated > 0
    if max_steps == 5:
        assert ref.n_truncated_only > 0
    s = ref.state()
    assert int((s["updates"] - start["updates"]).sum()) == n * T_RUN
    for p, name in ((0, act_a), (1, act_b)):
        k = "ab"[p]
        if name != "learn":                                         # a player that does not learn leaves R and Z alone
            assert (s["R_" + k] == 0.0).all() and (s["Z_" + k] == 0.0).all()
        else:
            assert s["R_" + k].tobytes() != start["R_" + k].tobytes() and s["Z_" + k].tobytes() != start["Z_" + k].tobytes()
            assert (s["Z_" + k] >= 0.0).all() and np.isfinite(s["R_" + k]).all()
            if plus:
                assert (s["R_" + k] >= 0.0).all() and not np.signbit(s["R_" + k]).any()      # never negative, never -0.0
            else:
                assert (s["R_" + k] < 0.0).any()
    d = ref.derived()
    for k in ("pi_a", "pi_b", "avg_a", "avg_b"):
        assert (d[k] >= 0.0).all() and np.abs(d[k].sum(2) - 1.0).max() < 1e-12


def test_every_branch_count_is_positive_over_the_cases():
    runs = [reference_run(*case)[1] for case in RUN_CASES]
    for k in ("n_uniform", "n_floor", "n_same", "n_terminated", "n_truncated_only"):
        assert sum(getattr(r, k) for r in runs) > 0, k


# ---- the vectorised restatement is n separate learners ----------------------------------------------------------------------
@pytest.mark.parametrize("modes, plus, linear", [(("learn", "learn"), True, False), (("learn", "learn"), False, True),
                                                 (("fixed", "learn"), True, True), (("learn", "uniform"), False, False)],
                         ids=["learn-learn plus", "learn-learn linear", "fixed per member-learn plus linear", "learn-uniform plain"])
def test_the_vectorised_restatement_is_n_separate_members_bit_for_bit(modes, plus, linear):
    """5x4, slip 0.2, 33 members, 200 steps, max_steps = 6 so that episodes truncate; per-member arrays for all four
    hyperparameters; a fixed player A has a policy per member.  Member i alone is a one-member instance fed lane i's
    transitions through update()."""
    n, T = 33, 200
    rng = np.random.default_rng(5)
    hyper = dict(alpha=rng.uniform(0.3, 1.0, n), decay=rng.uniform(0.95, 1.0, n), explor=rng.uniform(0.05, 0.6, n))
    gam = rng.uniform(0.5, 0.95, n)
    o = Oracle(5, 4, 0.2, n=n, seed=1994, autoreset=True, max_steps=6)
    fixed = rng.dirichlet(np.ones(5), (n, o.nS))
    acts = lambda i: tuple((fixed if i is None else fixed[i]) if m == "fixed" else m for m in modes)  # noqa: E731
    pop = RegretPopulationNumpy(n, o.nS, gam, q_init=0.3, plus=plus, linear=linear, act_a=acts(None)[0], act_b=acts(None)[1], **hyper)
    solo = [RegretPopulationNumpy(1, o.nS, gam[i], q_init=0.3, plus=plus, linear=linear, act_a=acts(i)[0], act_b=acts(i)[1],
                                  **{k: v[i] for k, v in hyper.items()}) for i in range(n)]
    obs = o.reset()
    for _ in range(T):
        for p in (0, 1):                                            # the rows the population draws from are the members' own
            rows = [q._rows(p, obs[i:i + 1]) for i, q in enumerate(solo)]
            if rows[0] is None:
                assert pop._rows(p, obs) is None
            else:
                np.testing.assert_array_equal(np.concatenate(rows), pop._rows(p, obs))
        a, b = o.sample_actions_mixed(np.arange(n), pop._rows(0, obs), pop._rows(1, obs))
        out = o.step(a, b)
        for i, q in enumerate(solo):        # every lane is live here (reset above, obs never 0 on an auto-reset handle)
            q.update(obs[i:i + 1], a[i:i + 1], b[i:i + 1], out["reward"][i:i + 1], out["terminated"][i:i + 1], out["final_obs"][i:i + 1])
        same = out["final_obs"] == obs; term = out["terminated"] != 0
        pop.n_same += int(same.sum()); pop.n_terminated += int(term.sum()); pop.n_truncated_only += int((~term & (out["truncated"] != 0)).sum())
        pop.update(obs, a, b, out["reward"], out["terminated"], out["final_obs"])
        obs = out["obs"]
        assert (obs != 0).all()
    assert pop.n_same > 0 and pop.n_terminated > 0 and pop.n_truncated_only > 0, (pop.n_same, pop.n_terminated, pop.n_truncated_only)
    want = {k: np.concatenate([q.state()[k] for q in solo]) for k in ROWS + ("updates", "alpha")}
    want["steps"] = solo[0].steps
    assert_regret_population_equal(pop.state(), want)
    assert (pop.n_uniform, pop.n_floor, pop.n_learned) == tuple(sum(getattr(q, k) for q in solo) for k in ("n_uniform", "n_floor", "n_learned"))
    assert pop.steps == T and pop.n_learned == n * T == int(pop.updates.sum()) and pop.n_uniform > 0 and (pop.n_floor > 0) == plus
    if plus:
        assert all((R >= 0.0).all() and not np.signbit(R).any() for R in pop.R)
    # run() is the same loop: a second population driven by run() on a second oracle ends in the same bits
    o2 = Oracle(5, 4, 0.2, n=n, seed=1994, autoreset=True, max_steps=6)
    pop2 = RegretPopulationNumpy(n, o2.nS, gam, q_init=0.3, plus=plus, linear=linear, act_a=acts(None)[0], act_b=acts(None)[1], **hyper)
    pop2.run(o2, o2.reset(), T)
    assert_regret_population_equal(pop2.state(), pop.state())
    assert (pop2.n_same, pop2.n_terminated, pop2.n_truncated_only, pop2.n_left_out) == (pop.n_same, pop.n_terminated, pop.n_truncated_only, 0)
    assert (pop2.n_uniform, pop2.n_floor, pop2.n_learned) == (pop.n_uniform, pop.n_floor, pop.n_learned)


def test_one_member_by_hand():
    """Member 1 of three, alpha = 0.5, gamma = 0.5, q_init = 0.25, (learn, uniform), plus and linear.  First update, at s = 2 with
    s' = 3: R = 0 everywhere so both policies are the 0.2 fallback; v = the ordered sum of five 0.2 * 0.25; Q_a[2][1] moves half
    way to m = 0 + 0.5 * v; u and the regrets follow; the floor zeroes the one negative regret, the moved action's.  Second update
    at the same state, terminated with r = +1: pi is now a quarter on each of the other four actions, there is no bootstrap, and
    n = 2 weighs the policy sum."""
    q = RegretPopulationNumpy(3, 4, 0.5, alpha=0.5, decay=0.5, explor=0.2, q_init=0.25, plus=True, linear=True, act_a="learn", act_b="uniform")
    one = dict(obs=[2, 2, 3], act_a=[1, 1, 0], act_b=[0, 0, 0], reward=[0, 0, 0], terminated=[0, 0, 0], next_obs=[3, 3, 1])
    q.update(keep=[False, True, False], **one)
    v = 0.0
    for _ in range(5):
        v = v + 0.2 * 0.25
    m_a = 0.0 + 0.5 * v
    qa = 0.25 + 0.5 * (m_a - 0.25)
    assert q.Q_a[1, 2].tolist() == [0.25, qa, 0.25, 0.25, 0.25] and q.Q_b[1, 2].tolist() == [0.25 + 0.5 * ((-0.0 + 0.5 * v) - 0.25)] + [0.25] * 4
    row = [0.25, qa, 0.25, 0.25, 0.25]
    u = 0.0
    for k in range(5):
        u = u + 0.2 * row[k]
    assert qa < u < 0.25
    up = 0.0 + (0.25 - u)
    assert q.R[0][1, 2].tolist() == [up, 0.0, up, up, up] and q.Z[0][1, 2].tolist() == [0.0 + 1.0 * 0.2] * 5
    assert q.updates.tolist() == [[0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]] and (q.n_uniform, q.n_floor, q.n_learned) == (2, 1, 1)
    assert (q.R[1] == 0.0).all() and (q.Z[1] == 0.0).all() and q.alpha.tolist() == [0.25, 0.25, 0.25] and q.steps == 1
    # the second update: s' == s, terminated with r = +1 for member 1 this time, so no bootstrap and m = 1
    two = dict(obs=[2, 2, 3], act_a=[0, 0, 0], act_b=[0, 0, 0], reward=[0, 1, 0], terminated=[0, 1, 0], next_obs=[2, 2, 1])
    tot = (((0.0 + up) + 0.0) + up) + up + up
    pi = [up / tot, 0.0, up / tot, up / tot, up / tot]
    q.update(keep=[False, True, False], **two)
    q0 = 0.25 + 0.25 * (1.0 - 0.25)
    row = [q0, qa, 0.25, 0.25, 0.25]
    u = 0.0
    for k in range(5):
        u = u + pi[k] * row[k]
    want = [up + (row[k] - u) for k in range(5)]
    want = [x if x > 0.0 else 0.0 for x in want]
    assert q.Q_a[1, 2].tolist() == row and q.R[0][1, 2].tolist() == want and want[1] == 0.0 and want[0] > up
    assert q.Z[0][1, 2].tolist() == [0.2 + 2.0 * pi[k] for k in range(5)]
    assert q.updates[1, 2] == 2 and q.alpha.tolist() == [0.125] * 3 and q.steps == 2 and q.n_learned == 2
    # nothing else moved: the members left out, the other states
    assert (q.Q_a[0, 1:] == 0.25).all() and (q.Q_a[2, 1:] == 0.25).all() and (q.R[0][[0, 2]] == 0.0).all() and (q.R[0][1, [0, 1, 3]] == 0.0).all()


def test_the_derived_rows():
    R = np.array([[1.0, -2.0, 3.0, 0.0, -0.0], [-1.0, -1.0, 0.0, -0.0, -5.0], [0.0, 0.0, 0.0, 0.0, 1e-300]])
    pi, tot = policy(R)
    assert pi[0].tolist() == [0.25, 0.0, 0.75, 0.0, 0.0] and pi[1].tolist() == [0.2] * 5 and pi[2].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0]
    assert tot.tolist() == [4.0, 0.0, 1e-300]
    Z = np.array([[0.0] * 5, [1.0, 0.0, 0.0, 0.0, 3.0]])
    assert average(Z).tolist() == [[0.2] * 5, [0.25, 0.0, 0.0, 0.0, 0.75]]
    x = np.array([0.1, 0.2, 0.3, 0.4, 0.5])
    assert ordered_sum(x) == ((((0.0 + 0.1) + 0.2) + 0.3) + 0.4) + 0.5


# ---- learning ------------------------------------------------------------------------------------------------------------
# Player A LEARNs against a UNIFORM player B on 5x4 at slip 0, a learner per lane, alpha 1 -> 0.01 over the run, Q = 0 at the
# start, regret matching+ with plain averaging.  Graded on nothing but two exact evaluations (best_response_np.evaluate): the
# kick-off value of the member's average policy avg_a against a uniform B must, in the median over the members, exceed the
# kick-off value of a uniform A against a uniform B.  Measured with this restatement (learning_run below; 16 members, 4 000
# steps, 6 s on one core): the figures are in the test's output and in DESIGN.md section 25.
LEARN = dict(width=5, height=4, slip=0.0, gamma=0.9, n=16, T=4000, seed=1994, explor=0.2, q_init=0.0, alpha=1.0)


def learning_run(seed=LEARN["seed"], T=LEARN["T"], n=LEARN["n"], plus=True, linear=False):
    """(the population after T steps, the kick-off value of every member's avg_a and of its pi_a against a uniform B, the
    kick-off value of uniform against uniform)"""
    c = LEARN
    o = Oracle(c["width"], c["height"], c["slip"], n=n, seed=seed, autoreset=True)
    lists = shapley_lists(Oracle(c["width"], c["height"], c["slip"], n=4, seed=seed, autoreset=True))
    starts = isd_obs(o)
    uniform = np.full((o.nS, 5), 0.2)
    q = RegretPopulationNumpy(n, o.nS, c["gamma"], alpha=c["alpha"], decay=0.01 ** (1.0 / T), explor=c["explor"], q_init=c["q_init"],
                              plus=plus, linear=linear, act_a="learn", act_b="uniform")
    q.run(o, o.reset(), T)
    every = np.ascontiguousarray(np.broadcast_to(uniform, (n, o.nS, 5)))
    d = q.derived()
    v_avg = kickoff(br.evaluate(lists, d["avg_a"], every, c["gamma"], 1e-10)[0], starts)
    v_pi = kickoff(br.evaluate(lists, d["pi_a"], every, c["gamma"], 1e-10)[0], starts)
    v_uniform = kickoff(br.evaluate(lists, uniform, uniform, c["gamma"], 1e-10)[0], starts)[0]
    return q, v_avg, v_pi, float(v_uniform)


def test_the_average_policy_beats_a_uniform_player_a_against_a_uniform_b():
    c = LEARN
    t0 = time.perf_counter()
    q, v_avg, v_pi, v_uniform = learning_run()
    print("A learns, B uniform, %d members x %d steps, seed %d: kick-off value of avg_a, median %.6f (members %.6f .. %.6f); of pi_a, "
          "median %.6f; uniform against uniform %.6f; %.1f s" % (c["n"], c["T"], c["seed"], np.median(v_avg), v_avg.min(), v_avg.max(),
                                                                 np.median(v_pi), v_uniform, time.perf_counter() - t0))
    assert q.steps == c["T"] and np.abs(q.alpha - 0.01).max() < 1e-9 and q.n_left_out == 0 and int(q.updates.sum()) == c["n"] * c["T"]
    assert (q.R[1] == 0.0).all() and (q.Z[1] == 0.0).all()
    assert np.median(v_avg) > v_uniform
