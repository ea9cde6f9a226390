"""The regret matchers of one table of include/soccer_hip.h ("learners, regret matching") restated in numpy, step for step, on
top of the Q-learners' restatement (tests/q_learning_np.py): the run loop and the threshold tables are QLearningNumpy's; the
update is its own, because the bootstrap is the quantised value of the player's own policy where the parent's is the quantised
row maximum.  Step 5 is the definition's float64 arithmetic, one elementwise operation at a time over the touched states
(elementwise IEEE operations give each state what a scalar loop over it gives).  It also counts its branches.
tests/test_gpu_regret_matching.py holds the device to it bit for bit; tests/test_regret_matching_np.py checks the definition
and that it learns."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from q_learning_np import SCALE, QLearningNumpy, behaviour  # noqa: E402

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


def own_value(pi, Q):
    """v_p[s] = sum_k pi[s][k] * Q[s][k], accumulated from 0.0 in k order"""
    v = np.zeros(pi.shape[:-1])
    for k in range(5):
        v = v + pi[..., k] * Q[..., k]
    return v


class RegretMatchingNumpy(QLearningNumpy):
    """act_a / act_b: 'learn' (regret matching), 'uniform' (the null row table; the 0.2 rows) or a fixed [nS, 5] mixed policy.
    Q_b is in player B's own reward.  Both tables are always updated.  plus, linear: the flags of the definition."""

    def __init__(self, nS, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, plus=True, linear=False,
                 act_a="learn", act_b="learn"):
        super().__init__(nS, discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init, act_a=act_a, act_b=act_b)
        self.plus, self.linear = bool(plus), bool(linear)
        self.rows = [None if isinstance(x, str) else np.array(x, np.float64) for x in self.act]
        self.R = [np.zeros((nS, 5)), np.zeros((nS, 5))]
        self.Z = [np.zeros((nS, 5)), np.zeros((nS, 5))]
        self.updates = np.zeros(nS, np.uint64)
        # the branches of step 5: a touched LEARN row whose policy was the 0.2 fallback (tot not > 0); the floor of `plus`
        # changed a value; a regret left negative (plain regret matching)
        self.n_fallback = self.n_floor = self.n_negative = 0

    def learns(self, p):
        return isinstance(self.act[p], str) and self.act[p] == "learn"

    def policy(self, p):
        """policy(p, .) [nS, 5]"""
        if self.learns(p):
            return policy(self.R[p])[0]
        return np.full((self.nS, 5), 0.2) if self.rows[p] is None else self.rows[p]

    def _table(self, p):
        if self.learns(p):
            return behaviour(self.policy(p), self.explor)
        return super()._table(p)

    def update(self, obs, act_a, act_b, reward, terminated, next_obs):
        """steps 3-6 on a batch of transitions (all of them valid)"""
        nS = self.nS
        Q = (self.Q_a, self.Q_b)
        obs = np.asarray(obs).astype(np.int64); nxt = np.asarray(next_obs).astype(np.int64)
        cell = obs * 25 + np.asarray(act_a).astype(np.int64) * 5 + np.asarray(act_b).astype(np.int64)
        live = 1 - (np.asarray(terminated) != 0).astype(np.int64)
        # Vq_p as it stood at the end of the previous step: a function of the R and Q of that moment, which are still here
        Vq = [np.rint(own_value(self.policy(p), Q[p]) * SCALE).astype(np.int64) for p in (0, 1)]
        c = np.bincount(cell, minlength=nS * 25).astype(np.int64).reshape(nS, 5, 5)                      # step 3
        R = np.zeros(nS * 25, np.int64); np.add.at(R, cell, np.asarray(reward).astype(np.int64))
        SA = np.zeros(nS * 25, np.int64); np.add.at(SA, cell, Vq[0][nxt] * live)
        SB = np.zeros(nS * 25, np.int64); np.add.at(SB, cell, Vq[1][nxt] * live)
        R = R.reshape(nS, 5, 5); SA = SA.reshape(nS, 5, 5); SB = SB.reshape(nS, 5, 5)
        # step 4: player A sums over b, player B over a and in its own reward
        for q, cc, RR, SV in ((self.Q_a, c.sum(2), R.sum(2), SA.sum(2)), (self.Q_b, c.sum(1), -R.sum(1), SB.sum(1))):
            t = cc > 0
            m = (RR[t].astype(np.float64) + self.gamma * (SV[t].astype(np.float64) * 2.0 ** -40)) / cc[t].astype(np.float64)
            q[t] = q[t] + self.alpha * (m - q[t])
        self.visits += c.reshape(nS, 25).astype(np.uint64)
        t = np.unique(obs)                                                       # step 5: the states with a touched joint cell
        self.updates[t] += np.uint64(1)
        n = self.updates[t].astype(np.float64)
        w = n if self.linear else np.ones(t.size)
        for p in (0, 1):
            if not self.learns(p) or t.size == 0:
                continue
            pi, tot = policy(self.R[p][t])                                       # from R as it was before this step
            self.n_fallback += int((~(tot > 0.0)).sum())
            q = Q[p][t]                                                          # after step 4
            u = own_value(pi, q)
            x = self.R[p][t] + (q - u[:, None])
            if self.plus:
                self.n_floor += int((x < 0.0).sum())
                x = np.where(x > 0.0, x, 0.0)
            else:
                self.n_negative += int((x < 0.0).sum())
            self.R[p][t] = x
            self.Z[p][t] = self.Z[p][t] + w[:, None] * pi
        self.alpha = self.alpha * self.decay                                     # step 6
        self.steps += 1

    def state(self):
        return {"Q_a": self.Q_a, "Q_b": self.Q_b, "R_a": self.R[0], "R_b": self.R[1], "Z_a": self.Z[0], "Z_b": self.Z[1],
                "visits": self.visits, "updates": self.updates, "alpha": self.alpha, "steps": self.steps}

    def derived(self):
        """pi_a, pi_b, avg_a, avg_b as RegretLearner.read() derives them"""
        out = {}
        for p, name in enumerate("ab"):
            if self.learns(p):
                out["pi_" + name], out["avg_" + name] = policy(self.R[p])[0], average(self.Z[p])
            else:
                out["pi_" + name], out["avg_" + name] = self.policy(p).copy(), self.policy(p).copy()
        return out


def assert_regret_equal(got, want):
    """bit for bit: a learner's read() against another's, or against RegretMatchingNumpy.state()"""
    for k in ROWS:
        g = np.ascontiguousarray(got[k], np.float64).view(np.uint64); w = np.ascontiguousarray(want[k], np.float64).view(np.uint64)
        bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
        assert bad.size == 0, "%s differs in %d entries, first at flat index %d: %r vs %r" % (
            k, bad.size, bad[0], np.asarray(got[k]).reshape(-1)[bad[0]], np.asarray(want[k]).reshape(-1)[bad[0]])
    for k in ("visits", "updates"):
        np.testing.assert_array_equal(np.asarray(got[k], np.uint64), np.asarray(want[k], np.uint64), k)
    assert np.float64(got["alpha"]).view(np.uint64) == np.float64(want["alpha"]).view(np.uint64), (got["alpha"], want["alpha"])
    assert int(got["steps"]) == int(want["steps"])
