"""The vectorised numpy restatement of the population of Q-learners (tests/q_population_np.py) is n separate one-actor
Q-learners (tests/q_learning_np.py, member i fed lane i's transitions through update()) bit for bit, does what the definition
says on a hand case, and it learns: every member's values approach those of the exact best response to the uniform opponent
(tests/best_response_np.py).  tests/test_gpu_q_population.py pins the device to this restatement bit for bit, so this guards
the yardstick where there is no GPU."""
import os
import sys
import time

import numpy as np
import pytest

from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_response_np as br  # noqa: E402
from minimax_q_np import shapley_lists  # noqa: E402
from q_learning_np import QLearningNumpy, behaviour, greedy  # noqa: E402
from q_population_np import QPopulationNumpy, assert_population_equal  # noqa: E402

# the learning run of tests/test_gpu_q_population.py: QR (greedy A, uniform B), a learner per lane, alpha 1 -> 0.01 over the run
LEARN = dict(width=5, height=4, slip=0.0, gamma=0.9, n=64, T=150000, seed=1994, explor=0.2, q_init=0.0, alpha=1.0)
# Population mean (over the 64 members) of the mean over the 760 live states of |V_a - V(A's exact best response to a uniform
# B)|, measured with this restatement (learning_run below; the spread over the members in brackets: min .. max):
#   seed, slip     mean over members
#   1994, 0        0.282269  (0.210516 .. 0.389415)
#   1,    0        0.280030  (0.223601 .. 0.387803)
#   2,    0.2      0.233131  (0.198913 .. 0.281191)
#   7,    0.2      0.233345  (0.194586 .. 0.309528)
# T is 150 000, not Littman's 10^6: a run takes 50 s on one core.  One learner sees each of the 3 800 (state, action) pairs
# some forty times in it, so the values are still far from converged (0.57 after 20 000 steps, 0.28 here): the figure says that
# a member learns at the rate one stream of experience allows, not that it has arrived.
# The spread between seeds is the only noise, so the bound is twice the worst of the four (DESIGN section 12's rule).
BOUND = 2 * 0.282269


def learning_run(seed, slip, T=LEARN["T"], n=LEARN["n"]):
    """(the population after T steps, per-member mean error over the live states)"""
    c = LEARN
    o = Oracle(c["width"], c["height"], slip, n=n, seed=seed, autoreset=True)
    want = br.best_response(shapley_lists(o), np.full((o.nS, 5), 0.2), 1, c["gamma"], 1e-10)[1][0]      # A answers a uniform B
    q = QPopulationNumpy(n, o.nS, c["gamma"], alpha=c["alpha"], decay=0.01 ** (1.0 / T), explor=c["explor"], q_init=c["q_init"],
                         act_a="greedy", act_b="uniform")
    q.run(o, o.reset(), T)
    return q, np.abs(q.Q_a.max(2) - want)[:, 1:].mean(1)


def test_the_vectorised_restatement_is_n_separate_learners_bit_for_bit():
    """5x4, slip 0.2, 33 members, 200 steps, max_steps = 5 so that episodes truncate; QQ, so both rows follow the tables"""
    n, T, kw = 33, 200, dict(alpha=0.9, decay=0.99, explor=0.2, q_init=0.3)
    o = Oracle(5, 4, 0.2, n=n, seed=1994, autoreset=True, max_steps=5)
    pop = QPopulationNumpy(n, o.nS, 0.9, **kw)
    solo = [QLearningNumpy(o.nS, 0.9, **kw) for _ in range(n)]
    obs = o.reset()
    for _ in range(T):
        rows = [np.stack([behaviour(greedy((q.Q_a, q.Q_b)[p][s:s + 1]), 0.2)[0] for q, s in zip(solo, obs)]) for p in (0, 1)]
        for p in (0, 1):
            np.testing.assert_array_equal(rows[p], pop._rows(p, obs))       # the rows the population draws from are the members' own
        a, b = o.sample_actions_mixed(np.arange(n), rows[0], rows[1])
        out = o.step(a, b)
        for i, q in enumerate(solo):        # every lane is live here (reset above, obs never 0 on an auto-reset handle)
            q.update(obs[i:i + 1], a[i:i + 1], b[i:i + 1], out["reward"][i:i + 1], out["terminated"][i:i + 1], out["final_obs"][i:i + 1])
        same = out["final_obs"] == obs; term = out["terminated"] != 0
        pop.n_same += int(same.sum()); pop.n_terminated += int(term.sum()); pop.n_truncated_only += int((~term & (out["truncated"] != 0)).sum())
        pop.update(obs, a, b, out["reward"], out["terminated"], out["final_obs"])
        obs = out["obs"]
        assert (obs != 0).all()
    assert pop.n_same > 0 and pop.n_terminated > 0 and pop.n_truncated_only > 0, (pop.n_same, pop.n_terminated, pop.n_truncated_only)
    want = {"Q_a": np.stack([q.Q_a for q in solo]), "Q_b": np.stack([q.Q_b for q in solo]),
            "alpha": np.array([q.alpha for q in solo]), "steps": solo[0].steps}
    assert_population_equal(pop.state(), want)
    assert pop.steps == T and (np.abs(pop.Q_a - 0.3) > 0).sum() > n
    # run() is the same loop: a second population driven by run() on a second oracle ends in the same bits
    o2 = Oracle(5, 4, 0.2, n=n, seed=1994, autoreset=True, max_steps=5)
    pop2 = QPopulationNumpy(n, o2.nS, 0.9, **kw)
    pop2.run(o2, o2.reset(), T)
    assert_population_equal(pop2.state(), pop.state())
    assert (pop2.n_same, pop2.n_terminated, pop2.n_truncated_only, pop2.n_left_out) == (pop.n_same, pop.n_terminated, pop.n_truncated_only, 0)


def test_update_on_a_hand_case():
    """alpha = 1: member 0 stands still (s' == s: the bootstrap is the row's value BEFORE the update), member 1 scores"""
    q = QPopulationNumpy(3, 761, 0.9, alpha=1.0, decay=[0.5, 0.25, 1.0], q_init=0.5)
    q.Q_a[0, 7] = [0.1, 0.2, 0.7, 0.3, 0.4]; q.Q_b[0, 7] = [-0.1, -0.6, -0.2, -0.3, -0.4]
    q.update(obs=[7, 9, 5], act_a=[2, 4, 0], act_b=[1, 3, 0], reward=[0, 1, 0], terminated=[0, 1, 0], next_obs=[7, 0, 6],
             keep=[True, True, False])
    grid = lambda v: float(np.rint(v * 2.0 ** 40)) * 2.0 ** -40  # noqa: E731
    assert q.Q_a[0, 7, 2] == 0.7 + 1.0 * ((0.0 + 0.9 * grid(0.7)) - 0.7)
    assert q.Q_b[0, 7, 1] == -0.6 + 1.0 * ((-0.0 + 0.9 * grid(-0.1)) - -0.6)
    assert q.Q_a[1, 9, 4] == 1.0 and q.Q_b[1, 9, 3] == -1.0
    moved_a = np.zeros((3, 761, 5), bool); moved_a[0, 7] = True; moved_a[1, 9, 4] = True; moved_a[:, 0] = True
    moved_b = np.zeros((3, 761, 5), bool); moved_b[0, 7] = True; moved_b[1, 9, 3] = True; moved_b[:, 0] = True
    assert (q.Q_a[~moved_a] == 0.5).all() and (q.Q_b[~moved_b] == 0.5).all() and (q.Q_a[:, 0] == 0).all() and (q.Q_b[:, 0] == 0).all()
    assert q.Q_a[0, 7].tolist() == [0.1, 0.2, q.Q_a[0, 7, 2], 0.3, 0.4]
    assert q.alpha.tolist() == [0.5, 0.25, 1.0] and q.steps == 1      # the member left out advances its alpha too


def test_the_restatement_learns_the_best_response_values():
    c = LEARN
    t0 = time.perf_counter()
    q, err = learning_run(c["seed"], c["slip"])
    print("QR, %d members x %d steps, seed %d: population mean %.6f (members %.6f .. %.6f) of the mean over live states of "
          "|V_a - V(best response)|; %.1f s" % (c["n"], c["T"], c["seed"], err.mean(), err.min(), err.max(), time.perf_counter() - t0))
    assert q.steps == c["T"] and np.abs(q.alpha - 0.01).max() < 1e-9
    assert q.n_left_out == 0 and q.n_same > 0 and q.n_terminated > 0
    assert err.mean() <= BOUND
