"""The batched policy hill-climbers of include/soccer_hip.h ("learners, policy hill-climbing": PHC and WoLF-PHC) restated in
numpy, step for step, on top of the Q-learners' restatement (tests/q_learning_np.py): steps 1-4 and 6 are QLearningNumpy's, the
policy step is the definition's float64 arithmetic, one elementwise operation at a time over the touched states (elementwise
IEEE operations give each state what a scalar loop over it gives).  It also counts which way step 5 went.
tests/test_gpu_wolf_phc.py holds the device to it bit for bit; tests/test_wolf_phc_np.py checks the definition and that it learns."""
import numpy as np

from q_learning_np import QLearningNumpy, behaviour

ROWS = ("Q_a", "Q_b", "V_a", "V_b", "pi_a", "pi_b", "avg_a", "avg_b")


class WolfPHCNumpy(QLearningNumpy):
    """act_a / act_b: 'learn' (a hill-climbing mixed policy), 'uniform' (the null row table; pi = avg = 0.2) or a fixed [nS, 5]
    mixed policy (pi = avg = that policy).  Q_b is in player B's own reward.  Both tables are always updated."""

    def __init__(self, nS, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, delta_win=0.01,
                 delta_lose=0.04, delta_decay=1.0, act_a="learn", act_b="learn"):
        super().__init__(nS, discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init, act_a=act_a, act_b=act_b)
        self.delta_win, self.delta_lose, self.delta_decay = float(delta_win), float(delta_lose), float(delta_decay)
        self.dscale = 1.0
        self.pi = [np.full((nS, 5), 0.2) if isinstance(x, str) else np.array(x, np.float64) for x in self.act]
        self.avg = [x.copy() for x in self.pi]
        self.updates = np.zeros(nS, np.uint64)
        # step 5's branches: ep > ea, the other one, and min() returning a pi[k] with 0 < pi[k] < d
        self.n_win = self.n_lose = self.n_clamp = 0

    def learns(self, p):
        return isinstance(self.act[p], str) and self.act[p] == "learn"

    def _table(self, p):
        if self.learns(p):
            return behaviour(self.pi[p], self.explor)
        return super()._table(p)

    def update(self, obs, act_a, act_b, reward, terminated, next_obs):
        """steps 3-6 on a batch of transitions (all of them valid)"""
        super().update(obs, act_a, act_b, reward, terminated, next_obs)          # steps 3, 4 and alpha / steps of 6
        t = np.unique(np.asarray(obs).astype(np.int64))                          # the states with a touched joint cell
        self.updates[t] += np.uint64(1)
        n = self.updates[t].astype(np.float64)
        for p in (0, 1):
            if not self.learns(p) or t.size == 0:
                continue
            Q = (self.Q_a, self.Q_b)[p][t]
            pi, avg = self.pi[p][t], self.avg[p][t]
            for k in range(5):
                avg[:, k] = avg[:, k] + (pi[:, k] - avg[:, k]) / n
            ep = np.zeros(t.size); ea = np.zeros(t.size)
            for k in range(5):
                ep = ep + pi[:, k] * Q[:, k]
                ea = ea + avg[:, k] * Q[:, k]
            win = ep > ea
            d = (np.where(win, self.delta_win, self.delta_lose) * self.dscale) / 4.0
            g = Q.argmax(1)                                                      # the first index that attains the maximum
            moved = np.zeros(t.size)
            for k in range(5):
                other = g != k
                m = np.where(other, np.minimum(pi[:, k], d), 0.0)
                self.n_clamp += int((other & (pi[:, k] > 0.0) & (pi[:, k] < d)).sum())
                pi[:, k] = np.where(other, pi[:, k] - m, pi[:, k])
                moved = np.where(other, moved + m, moved)
            rows = np.arange(t.size)
            pi[rows, g] = pi[rows, g] + moved
            self.pi[p][t] = pi; self.avg[p][t] = avg
            self.n_win += int(win.sum()); self.n_lose += int((~win).sum())
        self.dscale = self.dscale * self.delta_decay

    def state(self):
        return {"Q_a": self.Q_a, "Q_b": self.Q_b, "V_a": self.Q_a.max(1), "V_b": self.Q_b.max(1), "pi_a": self.pi[0], "pi_b": self.pi[1],
                "avg_a": self.avg[0], "avg_b": self.avg[1], "visits": self.visits, "updates": self.updates, "alpha": self.alpha,
                "dscale": self.dscale, "steps": self.steps}


def assert_phc_equal(got, want):
    """bit for bit: a learner's read() against another's, or against WolfPHCNumpy.state()"""
    for k in ROWS:
        g = np.ascontiguousarray(got[k], np.float64).view(np.uint64); w = np.ascontiguousarray(want[k], np.float64).view(np.uint64)
        bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
        assert bad.size == 0, "%s differs in %d entries, first at flat index %d: %r vs %r" % (
            k, bad.size, bad[0], np.asarray(got[k]).reshape(-1)[bad[0]], np.asarray(want[k]).reshape(-1)[bad[0]])
    for k in ("visits", "updates"):
        np.testing.assert_array_equal(np.asarray(got[k], np.uint64), np.asarray(want[k], np.uint64), k)
    for k in ("alpha", "dscale"):
        assert np.float64(got[k]).view(np.uint64) == np.float64(want[k]).view(np.uint64), (k, got[k], want[k])
    assert int(got["steps"]) == int(want["steps"])
