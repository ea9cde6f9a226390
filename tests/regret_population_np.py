"""The population of regret matchers of include/soccer_hip.h ("learners, a population of regret matchers") restated in numpy,
vectorised over the members: tables [n, nS, 5], member i fed by lane i of the oracle alone, one elementwise float64 operation
at a time in the definition's order.  The run loop, the hyperparameters and the counters of what a run met are
QPopulationNumpy's (tests/q_population_np.py); the update is its own (the bootstrap is the value of the player's own policy,
not the quantised maximum).  It also counts its branches.  tests/test_regret_population_np.py holds it to n separate
one-member instances bit for bit and checks that it learns; tests/test_gpu_regret_population.py holds the device to it bit
for bit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from q_learning_np import thresholds  # noqa: E402
from q_population_np import QPopulationNumpy  # noqa: E402

ROWS = ("Q_a", "Q_b", "R_a", "R_b", "Z_a", "Z_b")


def ordered_sum(x):
    """(((((0.0 + x[..., 0]) + x[..., 1]) + x[..., 2]) + x[..., 3]) + x[..., 4])"""
    tot = np.zeros(x.shape[:-1])
    for k in range(5):
        tot = tot + x[..., k]
    return tot


def policy(R):
    """policy(p, s) of a LEARN player: regrets [..., 5] -> (pi [..., 5], tot [...])"""
    pos = np.where(R > 0.0, R, 0.0)
    tot = ordered_sum(pos)
    safe = np.where(tot > 0.0, tot, 1.0)
    return np.where((tot > 0.0)[..., None], pos / safe[..., None], 0.2), tot


def average(Z):
    """avg_p: policy sums [..., 5] -> Z / (the row's ordered sum), 0.2 where that sum is 0"""
    tot = ordered_sum(Z)
    return np.where((tot == 0.0)[..., None], 0.2, Z / np.where(tot == 0.0, 1.0, tot)[..., None])


class RegretPopulationNumpy(QPopulationNumpy):
    """act_a / act_b: 'learn', 'uniform', a fixed [nS, 5] mixed policy for every member or [n, nS, 5], one per member.
    discount_factor, alpha, decay and explor: scalars, or arrays of n.  plus, linear: flags of the whole population."""

    def __init__(self, n, nS, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, plus=True, linear=False,
                 act_a="learn", act_b="learn"):
        super().__init__(n, nS, discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init, act_a="uniform", act_b="uniform")
        self.plus, self.linear = bool(plus), bool(linear)
        self.act = (act_a, act_b)
        self.rows = [None if isinstance(x, str) else np.broadcast_to(np.asarray(x, np.float64), (self.n, self.nS, 5)).copy() for x in self.act]
        self.R = [np.zeros((self.n, self.nS, 5)), np.zeros((self.n, self.nS, 5))]
        self.Z = [np.zeros((self.n, self.nS, 5)), np.zeros((self.n, self.nS, 5))]
        self.updates = np.zeros((self.n, self.nS), np.uint64)
        # the branches: policy() of a LEARN player fell back to 0.2 (tot = 0) at s or at s'; the floor of `plus` changed a
        # value; learned transitions
        self.n_uniform = self.n_floor = self.n_learned = 0

    def learns(self, p):
        return isinstance(self.act[p], str) and self.act[p] == "learn"

    def policy(self, p, i, s):
        """policy(p, s[j]) of member i[j]: [len(i), 5]"""
        if self.learns(p):
            pi, tot = policy(self.R[p][i, s])
            self.n_uniform += int((tot <= 0.0).sum())
            return pi
        if self.rows[p] is None:
            return np.full((len(i), 5), 0.2)
        return self.rows[p][i, s]

    def _rows(self, p, obs):
        """the draw of player p: every member's threshold row at its lane's observation, [n, 4] (None: the null row table)"""
        if isinstance(self.act[p], str) and self.act[p] == "uniform":
            return None
        count = self.n_uniform
        pi = self.policy(p, self.lanes, np.asarray(obs).astype(np.int64))
        self.n_uniform = count                                      # (the draw is not a branch of the update)
        e = self.explor[:, None] if self.learns(p) else 0.0        # a fixed player: its own row, explor 0
        return thresholds((1.0 - e) * pi + e / 5.0)

    def update(self, obs, act_a, act_b, reward, terminated, next_obs, keep=None):
        """steps 1-5, transition i for member i; members outside `keep` (bool [n]) leave their rows alone, every alpha advances"""
        i = self.lanes if keep is None else self.lanes[np.asarray(keep, bool)]
        s = np.asarray(obs).astype(np.int64)[i]; s2 = np.asarray(next_obs).astype(np.int64)[i]
        term = np.asarray(terminated)[i] != 0
        r = np.asarray(reward).astype(np.int64)[i]
        Q = (self.Q_a, self.Q_b)
        # step 1: both policies at s and at s', and Q at s', read before anything moves (s' may be s)
        pi = [self.policy(p, i, s) for p in (0, 1)]
        npi = [self.policy(p, i, s2) for p in (0, 1)]
        nq = [Q[p][i, s2].copy() for p in (0, 1)]
        for p, act, rp in ((0, act_a, r), (1, act_b, -r)):          # step 2
            v = np.zeros(i.size)
            for k in range(5):
                v = v + npi[p][:, k] * nq[p][:, k]
            v = np.where(term, 0.0, v)
            m = rp.astype(np.float64) + self.gamma[i] * v
            k = np.asarray(act).astype(np.int64)[i]
            old = Q[p][i, s, k]
            Q[p][i, s, k] = old + self.alpha[i] * (m - old)
        self.updates[i, s] += np.uint64(1)                          # step 3
        n = self.updates[i, s].astype(np.float64)
        w = n if self.linear else np.ones(i.size)
        for p in (0, 1):                                            # step 4
            if not self.learns(p) or i.size == 0:
                continue
            q = Q[p][i, s]
            u = np.zeros(i.size)
            for k in range(5):
                u = u + pi[p][:, k] * q[:, k]
            x = self.R[p][i, s] + (q - u[:, None])
            if self.plus:
                self.n_floor += int((x < 0.0).sum())
                x = np.where(x > 0.0, x, 0.0)
            self.R[p][i, s] = x
            self.Z[p][i, s] = self.Z[p][i, s] + w[:, None] * pi[p]
        self.n_learned += int(i.size)
        self.alpha = self.alpha * self.decay                        # step 5
        self.steps += 1

    def load(self, rng, max_updates=4):
        """The loaded state of the branch-coverage cases: Q uniform in [-1, 1]; regrets of mixed signs (none negative under
        plus), a fifth of the rows all <= 0 and exact zeros sprinkled in; policy sums with a fifth of the rows zero; small
        update counts (rows 0 stay what creation gave them).  Returns what RegretPopulation.load takes."""
        n, nS = self.n, self.nS
        self.Q_a[:, 1:] = rng.uniform(-1.0, 1.0, (n, nS - 1, 5)); self.Q_b[:, 1:] = rng.uniform(-1.0, 1.0, (n, nS - 1, 5))
        for p in (0, 1):
            if not self.learns(p):
                continue
            R = rng.uniform(-1.0, 1.0, (n, nS - 1, 5))
            R = np.where(rng.random((n, nS - 1, 1)) < 0.2, -np.abs(R), R)          # rows all <= 0
            R = np.where(rng.random((n, nS - 1, 5)) < 0.15, 0.0, R)                # exact zeros
            if self.plus:
                R = np.where(R > 0.0, R, 0.0)
            Z = rng.uniform(0.0, 3.0, (n, nS - 1, 5)) * (rng.random((n, nS - 1, 1)) >= 0.2)
            self.R[p][:, 1:] = R; self.Z[p][:, 1:] = Z
        self.updates[:, 1:] = rng.integers(0, max_updates, (n, nS - 1)).astype(np.uint64)
        return {k: v.copy() for k, v in self.state().items() if k in ROWS + ("updates",)}

    def state(self, first=0, count=None):
        sl = slice(first, None if count is None else first + count)
        return {"Q_a": self.Q_a[sl], "Q_b": self.Q_b[sl], "R_a": self.R[0][sl], "R_b": self.R[1][sl], "Z_a": self.Z[0][sl],
                "Z_b": self.Z[1][sl], "updates": self.updates[sl], "alpha": self.alpha[sl], "steps": self.steps}

    def derived(self, first=0, count=None):
        """pi_a, pi_b, avg_a, avg_b as RegretPopulation.read() derives them"""
        sl = slice(first, None if count is None else first + count)
        out = {}
        for p, name in enumerate("ab"):
            if self.learns(p):
                out["pi_" + name], out["avg_" + name] = policy(self.R[p][sl])[0], average(self.Z[p][sl])
            else:
                rows = np.full((self.n, self.nS, 5), 0.2) if self.rows[p] is None else self.rows[p]
                out["pi_" + name], out["avg_" + name] = rows[sl].copy(), rows[sl].copy()
        return out


def assert_regret_population_equal(got, want):
    """bit for bit: a population's read() against another's, or against RegretPopulationNumpy.state()"""
    for k in ROWS + ("alpha",):
        g = np.ascontiguousarray(got[k], np.float64).view(np.uint64).reshape(-1)
        w = np.ascontiguousarray(want[k], np.float64).view(np.uint64).reshape(-1)
        assert g.shape == w.shape, (k, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s differs in %d entries, first at flat index %d: %r vs %r" % (
            k, bad.size, bad[0], np.asarray(got[k]).reshape(-1)[bad[0]], np.asarray(want[k]).reshape(-1)[bad[0]])
    np.testing.assert_array_equal(np.asarray(got["updates"], np.uint64), np.asarray(want["updates"], np.uint64), "updates")
    assert int(got["steps"]) == int(want["steps"])
