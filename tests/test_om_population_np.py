"""The vectorised numpy restatement of the population of opponent-modelling Q-learners (tests/om_population_np.py) is n
separate scalar-loop learners written straight from the text of include/soccer_hip.h ("learners, a population of
opponent-modelling Q-learners") bit for bit; its derive function does what the definition says at the edges (no observation,
a tie, a skewed count, the clamp); s' == s bootstraps from the value before the update; the two players' counts add up; and it
learns: every member's values approach those of the exact best response to the uniform opponent (tests/best_response_np.py).
tests/test_gpu_om_population.py pins the device to this restatement bit for bit, so this guards the yardstick where there is
no GPU."""
import os
import sys
import time

import numpy as np

from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_response_np as br  # noqa: E402
from minimax_q_np import shapley_lists  # noqa: E402
from om_population_np import OMPopulationNumpy, assert_om_population_equal, derive  # noqa: E402
from q_learning_np import SCALE, behaviour  # noqa: E402
from test_q_population_np import LEARN as Q_LEARN  # noqa: E402

# The learning run of tests/test_gpu_om_population.py: the LEARN protocol of tests/test_q_population_np.py — (greedy A, uniform
# B), a learner per lane, Q = 0, alpha 1 -> 0.01 over the run — with T = 100 000 steps, not LEARN's 150 000: this restatement
# derives V three times a step from joint-action rows and takes about 0.45 ms a step at n = 64, so 100 000 steps keep the run
# under a minute on one core.
LEARN = dict(Q_LEARN, T=100000)
# Population mean (over the 64 members) of the mean over the 760 live states of |V_a - V(A's exact best response to a uniform
# B)|, measured with this restatement (learning_run below; the spread over the members in brackets: min .. max):
#   seed, slip     mean over members
#   1994, 0        0.538784  (0.501422 .. 0.575797)
#   1,    0        0.538159  (0.496842 .. 0.575193)
#   2,    0.2      0.453875  (0.428706 .. 0.478748)
#   7,    0.2      0.453420  (0.431706 .. 0.472633)
# One learner sees each of the 19 000 (state, own action, other's action) cells some five times in such a run — a Q-learner of
# tests/test_q_population_np.py sees each of its 3 800 cells some forty times in its 150 000 steps and reaches 0.28 — so the
# values are far from converged (0.60 after 3 000 steps, 0.54 here): the figure says that a member learns at the rate one
# stream of experience allows a table five times as large, not that it has arrived.
# The spread between seeds is the only noise, so the bound is twice the worst of the four (DESIGN section 12's rule).  At
# this T that is a weak bound, above 1: it catches a learner that diverges or learns the wrong sign, not one that is slow.
BOUND = 2 * 0.538784


def learning_run(seed, slip, T=LEARN["T"], n=LEARN["n"]):
    """(the population after T steps, per-member mean error over the live states)"""
    c = LEARN
    o = Oracle(c["width"], c["height"], slip, n=n, seed=seed, autoreset=True)
    want = br.best_response(shapley_lists(o), np.full((o.nS, 5), 0.2), 1, c["gamma"], 1e-10)[1][0]      # A answers a uniform B
    q = OMPopulationNumpy(n, o.nS, c["gamma"], alpha=c["alpha"], decay=0.01 ** (1.0 / T), explor=c["explor"], q_init=c["q_init"],
                          act_a="greedy", act_b="uniform")
    q.run(o, o.reset(), T)
    return q, np.abs(derive(q.Q_a, q.C_a)[0] - want)[:, 1:].mean(1)


# ---- the definition, in loops --------------------------------------------------------------------------
def derive_loop(Q, C):
    """the header's expression for one (player, state), literally: Q[own][other] floats, C[other] ints -> (V, g, W[g] / N)"""
    n = C[0] + C[1] + C[2] + C[3] + C[4]
    w = [float(C[k]) if n > 0 else 1.0 for k in range(5)]
    N = float(n) if n > 0 else 5.0
    W = []
    for a in range(5):
        x = w[0] * Q[a][0]
        for k in range(1, 5):
            x = x + w[k] * Q[a][k]
        W.append(x)
    g = 0
    for a in range(1, 5):
        if W[a] > W[g]:
            g = a
    return min(1.0, max(-1.0, W[g] / N)), g, W[g] / N


class ScalarLearner:
    """one member, in Python floats and ints, step by step as the header words it"""

    def __init__(self, nS, gamma, alpha, decay, explor, q_init):
        self.gamma, self.alpha, self.decay, self.explor = gamma, alpha, decay, explor
        self.Q = [[[[0.0 if s == 0 else q_init for _ in range(5)] for _ in range(5)] for s in range(nS)] for _ in range(2)]
        self.C = [[[0] * 5 for _ in range(nS)] for _ in range(2)]
        self.steps = 0

    def row(self, p, s):
        g = derive_loop(self.Q[p][s], self.C[p][s])[1]
        return behaviour(np.eye(5)[g][None], self.explor)[0]

    def update(self, s, a, b, r, terminated, s2):
        sv = [0 if terminated else int(np.rint(derive_loop(self.Q[p][s2], self.C[p][s2])[0] * SCALE)) for p in (0, 1)]
        for p, own, other, R in ((0, a, b, r), (1, b, a, -r)):
            m = float(R) + self.gamma * (float(sv[p]) * 2.0 ** -40)
            q = self.Q[p][s][own][other]
            self.Q[p][s][own][other] = q + self.alpha * (m - q)
            self.C[p][s][other] += 1
        self.alpha = self.alpha * self.decay
        self.steps += 1


def test_the_vectorised_restatement_is_n_separate_scalar_learners_bit_for_bit():
    """5x4, slip 0.2, 33 members, 200 steps, max_steps = 5 so that episodes truncate; both players greedy, so both rows follow
    the tables and the counts"""
    n, T, kw = 33, 200, dict(alpha=0.9, decay=0.99, explor=0.2, q_init=0.3)
    o = Oracle(5, 4, 0.2, n=n, seed=1994, autoreset=True, max_steps=5)
    pop = OMPopulationNumpy(n, o.nS, 0.9, **kw)
    solo = [ScalarLearner(o.nS, 0.9, **kw) for _ in range(n)]
    obs = o.reset()
    for _ in range(T):
        rows = [np.stack([q.row(p, int(s)) for q, s in zip(solo, obs)]) for p in (0, 1)]
        for p in (0, 1):
            np.testing.assert_array_equal(rows[p], pop._rows(p, obs))       # the rows the population draws from are the members' own
        a, b = o.sample_actions_mixed(np.arange(n), rows[0], rows[1])
        out = o.step(a, b)
        for i, q in enumerate(solo):        # every lane is live here (reset above, obs never 0 on an auto-reset handle)
            q.update(int(obs[i]), int(a[i]), int(b[i]), int(out["reward"][i]), bool(out["terminated"][i]), int(out["final_obs"][i]))
        pop.update(obs, a, b, out["reward"], out["terminated"], out["final_obs"])
        obs = out["obs"]
        assert (obs != 0).all()
    want = {"Q_a": np.array([q.Q[0] for q in solo]), "Q_b": np.array([q.Q[1] for q in solo]),
            "C_a": np.array([q.C[0] for q in solo], np.uint64), "C_b": np.array([q.C[1] for q in solo], np.uint64),
            "alpha": np.array([q.alpha for q in solo]), "steps": solo[0].steps}
    assert_om_population_equal(pop.state(), want)
    assert pop.steps == T and (np.abs(pop.Q_a - 0.3) > 0).sum() > n and pop.n_first_seen > 0
    # run() is the same loop: a second population driven by run() on a second oracle ends in the same bits
    o2 = Oracle(5, 4, 0.2, n=n, seed=1994, autoreset=True, max_steps=5)
    pop2 = OMPopulationNumpy(n, o2.nS, 0.9, **kw)
    pop2.run(o2, o2.reset(), T)
    assert_om_population_equal(pop2.state(), pop.state())
    assert pop2.n_same > 0 and pop2.n_terminated > 0 and pop2.n_truncated_only > 0 and pop2.n_left_out == 0
    assert pop2.n_first_seen == pop.n_first_seen


def _both(Q, C):
    """the vectorised derive and the literal loop on one row: they agree to the bit; returns the loop's (V, g, W[g] / N)"""
    V, g = derive(np.array(Q, np.float64), np.array(C, np.uint64))
    want = derive_loop(Q, C)
    assert np.float64(V).tobytes() == np.float64(want[0]).tobytes() and int(g) == want[1]
    return want


def test_derive_at_its_edges():
    rng = np.random.default_rng(5)
    Q = rng.uniform(-1.0, 1.0, (5, 5)).tolist()
    # nothing seen yet: a uniform belief, the row means
    V, g, _ = _both(Q, [0] * 5)
    means = [((((1.0 * r[0] + 1.0 * r[1]) + 1.0 * r[2]) + 1.0 * r[3]) + 1.0 * r[4]) / 5.0 for r in Q]
    assert V == max(means) and g == means.index(max(means))
    # a tie between actions: the first index wins
    tie = [[0.25] * 5, [0.5] * 5, [-1.0] * 5, [0.5] * 5, [0.5] * 5]
    assert _both(tie, [2, 0, 7, 0, 1])[:2] == (0.5, 1)
    assert _both([[0.3] * 5] * 5, [0] * 5)[1] == 0 and _both([[0.0] * 5] * 5, [4, 4, 4, 4, 4])[:2] == (0.0, 0)
    # counts (3, 0, 0, 0, 1): only columns 0 and 4 weigh
    V, g, _ = _both(Q, [3, 0, 0, 0, 1])
    W = [(((3.0 * r[0] + 0.0 * r[1]) + 0.0 * r[2]) + 0.0 * r[3]) + 1.0 * r[4] for r in Q]
    assert g == W.index(max(W)) and V == max(W) / 4.0
    # the clamp: beyond 2^53 the counts round one by one — 2^53 + 3 up to 2^53 + 4, and n = 2^53 + 5 down to 2^53 + 4 — so a row
    # of ones has W[g] / N = (2^53 + 6) / (2^53 + 4) > 1
    ones = [[1.0] * 5] + [[0.5] * 5] * 4
    V, g, ratio = _both(ones, [2 ** 53 + 3, 2, 0, 0, 0])
    assert ratio > 1.0 and V == 1.0 and g == 0
    V, g, ratio = _both([[-1.0] * 5] * 5, [2 ** 53 + 3, 2, 0, 0, 0])
    assert ratio < -1.0 and V == -1.0 and g == 0
    # many rows at once are the rows one by one
    Qs = rng.uniform(-1.0, 1.0, (40, 5, 5)); Cs = rng.integers(0, 4, (40, 5)).astype(np.uint64); Cs[::7] = 0
    Vs, gs = derive(Qs, Cs)
    for i in range(40):
        want = derive_loop(Qs[i].tolist(), [int(x) for x in Cs[i]])
        assert Vs[i] == want[0] and gs[i] == want[1]


def test_update_on_a_hand_case():
    """alpha = 1: member 0 stands still (s' == s: the bootstrap is the value BEFORE the update), member 1 scores at a state it
    has seen before, member 2 is left out"""
    q = OMPopulationNumpy(3, 761, 0.9, alpha=1.0, decay=[0.5, 0.25, 1.0], q_init=0.5)
    rng = np.random.default_rng(9)
    q.Q_a[0, 7] = rng.uniform(-1, 1, (5, 5)); q.Q_b[0, 7] = rng.uniform(-1, 1, (5, 5))
    q.C_a[0, 7] = [1, 0, 2, 0, 0]; q.C_b[0, 7] = [0, 0, 3, 0, 0]; q.C_a[1, 9] = [0, 0, 0, 1, 0]; q.C_b[1, 9] = [0, 0, 0, 0, 1]
    before = {k: v.copy() for k, v in q.state().items() if k != "steps"}
    va = derive_loop(before["Q_a"][0, 7].tolist(), [1, 0, 2, 0, 0])[0]; vb = derive_loop(before["Q_b"][0, 7].tolist(), [0, 0, 3, 0, 0])[0]
    q.update(obs=[7, 9, 5], act_a=[2, 4, 0], act_b=[1, 3, 0], reward=[0, 1, 0], terminated=[0, 1, 0], next_obs=[7, 0, 6],
             keep=[True, True, False])
    grid = lambda v: float(np.rint(v * 2.0 ** 40)) * 2.0 ** -40  # noqa: E731
    old_a, old_b = before["Q_a"][0, 7, 2, 1], before["Q_b"][0, 7, 1, 2]
    assert q.Q_a[0, 7, 2, 1] == old_a + 1.0 * ((0.0 + 0.9 * grid(va)) - old_a)
    assert q.Q_b[0, 7, 1, 2] == old_b + 1.0 * ((-0.0 + 0.9 * grid(vb)) - old_b)
    assert derive(q.Q_a[0, 7], q.C_a[0, 7])[0] != va                    # the value moved: it was read before
    assert q.C_a[0, 7].tolist() == [1, 1, 2, 0, 0] and q.C_b[0, 7].tolist() == [0, 0, 4, 0, 0]
    assert q.Q_a[1, 9, 4, 3] == 1.0 and q.Q_b[1, 9, 3, 4] == -1.0
    assert q.C_a[1, 9].tolist() == [0, 0, 0, 2, 0] and q.C_b[1, 9].tolist() == [0, 0, 0, 0, 2]
    for k, Q in (("Q_a", q.Q_a), ("Q_b", q.Q_b)):
        assert (Q != before[k]).sum() == 2 and (Q[:, 0] == 0).all() and (Q[2] == before[k][2]).all()
    assert (q.C_a[2] == 0).all() and (q.C_b[2] == 0).all() and q.C_a.sum() == before["C_a"].sum() + 2
    assert q.alpha.tolist() == [0.5, 0.25, 1.0] and q.steps == 1 and q.n_first_seen == 0      # the member left out advances its alpha too


def test_the_counts_of_the_two_players_add_up():
    """every kept transition adds one to a count of each player at its state"""
    n, T = 17, 120
    o = Oracle(5, 4, 0.2, n=n, seed=3, autoreset=True, max_steps=7)
    q = OMPopulationNumpy(n, o.nS, 0.9, alpha=0.5, decay=0.999, q_init=0.0, act_b="uniform")
    q.run(o, o.reset(), T)
    np.testing.assert_array_equal(q.C_a.sum(2), q.C_b.sum(2))
    assert int(q.C_a.sum()) == n * T - q.n_left_out == n * T and (q.C_a[:, 0] == 0).all() and (q.C_b[:, 0] == 0).all()
    assert q.n_first_seen == int((q.C_a.sum(2) > 0).sum())             # a state's first update, once per (member, state)
    assert np.abs(q.Q_a).max() <= 1.0 and np.abs(q.Q_b).max() <= 1.0


def test_the_restatement_learns_the_best_response_values():
    c = LEARN
    t0 = time.perf_counter()
    q, err = learning_run(c["seed"], c["slip"])
    print("(greedy, uniform), %d members x %d steps, seed %d: population mean %.6f (members %.6f .. %.6f) of the mean over live "
          "states of |V_a - V(best response)|; %.1f s" % (c["n"], c["T"], c["seed"], err.mean(), err.min(), err.max(), time.perf_counter() - t0))
    assert q.steps == c["T"] and np.abs(q.alpha - 0.01).max() < 1e-9
    assert q.n_left_out == 0 and q.n_same > 0 and q.n_terminated > 0 and q.n_first_seen > 0
    assert err.mean() <= BOUND
