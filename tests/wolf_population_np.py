"""The population of policy hill-climbers of include/soccer_hip.h ("learners, a population of policy hill-climbers") restated
in numpy, vectorised over the members: tables [n, nS, 5], member i fed by lane i of the oracle alone.  The Q update is
QPopulationNumpy's (tests/q_population_np.py), the policy step is WolfPHCNumpy's (tests/wolf_phc_np.py) with the member as the
leading axis, one elementwise float64 operation at a time.  It also counts which way the policy step went.
tests/test_wolf_population_np.py holds it to n separate WolfPHCNumpy instances bit for bit and checks that it learns;
tests/test_gpu_wolf_population.py holds the device to it bit for bit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from q_learning_np import thresholds  # noqa: E402
from q_population_np import QPopulationNumpy  # noqa: E402

ROWS = ("Q_a", "Q_b", "pi_a", "pi_b", "avg_a", "avg_b")


class WolfPopulationNumpy(QPopulationNumpy):
    """act_a / act_b: 'learn', 'uniform', a fixed [nS, 5] mixed policy for every member or [n, nS, 5], one per member.  The
    seven hyperparameters: scalars, or arrays of n."""

    def __init__(self, n, nS, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, delta_win=0.01,
                 delta_lose=0.04, delta_decay=1.0, act_a="learn", act_b="learn"):
        super().__init__(n, nS, discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init, act_a="uniform", act_b="uniform")
        per = lambda x: np.broadcast_to(np.asarray(x, np.float64), (self.n,)).copy()  # noqa: E731
        self.delta_win, self.delta_lose, self.delta_decay = per(delta_win), per(delta_lose), per(delta_decay)
        self.dscale = np.ones(self.n)
        self.act = (act_a, act_b)
        self.pi = [np.full((self.n, self.nS, 5), 0.2) if isinstance(x, str) else np.broadcast_to(np.asarray(x, np.float64), (self.n, self.nS, 5)).copy()
                   for x in self.act]
        self.avg = [x.copy() for x in self.pi]
        self.updates = np.zeros((self.n, self.nS), np.uint64)
        # the policy step's branches: ep > ea, the other one, and min() returning a pi[k] with 0 < pi[k] < d
        self.n_win = self.n_lose = self.n_clamp = 0

    def learns(self, p):
        return isinstance(self.act[p], str) and self.act[p] == "learn"

    def _rows(self, p, obs):
        """step 1 for player p: every member's threshold row at its lane's observation, [n, 4] (None: the null row table)"""
        if isinstance(self.act[p], str) and self.act[p] == "uniform":
            return None
        pi = self.pi[p][self.lanes, obs]
        e = self.explor[:, None] if self.learns(p) else 0.0        # a fixed player: its own row, explor 0
        return thresholds((1.0 - e) * pi + e / 5.0)

    def update(self, obs, act_a, act_b, reward, terminated, next_obs, keep=None):
        """steps 3-6, transition i for member i; members outside `keep` (bool [n]) leave their rows alone, every alpha and
        dscale advances"""
        super().update(obs, act_a, act_b, reward, terminated, next_obs, keep)    # steps 3, 4 and alpha / steps of 6
        i = self.lanes if keep is None else self.lanes[np.asarray(keep, bool)]
        s = np.asarray(obs).astype(np.int64)[i]
        self.updates[i, s] += np.uint64(1)
        n = self.updates[i, s].astype(np.float64)
        for p in (0, 1):
            if not self.learns(p) or i.size == 0:
                continue
            Q = (self.Q_a, self.Q_b)[p][i, s]
            pi, avg = self.pi[p][i, s], self.avg[p][i, s]
            for k in range(5):
                avg[:, k] = avg[:, k] + (pi[:, k] - avg[:, k]) / n
            ep = np.zeros(i.size); ea = np.zeros(i.size)
            for k in range(5):
                ep = ep + pi[:, k] * Q[:, k]
                ea = ea + avg[:, k] * Q[:, k]
            win = ep > ea
            d = (np.where(win, self.delta_win[i], self.delta_lose[i]) * self.dscale[i]) / 4.0
            g = Q.argmax(1)                                                      # the first index that attains the maximum
            moved = np.zeros(i.size)
            for k in range(5):
                other = g != k
                m = np.where(other, np.minimum(pi[:, k], d), 0.0)
                self.n_clamp += int((other & (pi[:, k] > 0.0) & (pi[:, k] < d)).sum())
                pi[:, k] = np.where(other, pi[:, k] - m, pi[:, k])
                moved = np.where(other, moved + m, moved)
            rows = np.arange(i.size)
            pi[rows, g] = pi[rows, g] + moved
            self.pi[p][i, s] = pi; self.avg[p][i, s] = avg
            self.n_win += int(win.sum()); self.n_lose += int((~win).sum())
        self.dscale = self.dscale * self.delta_decay

    def load(self, rng, max_updates=4):
        """the loaded state of the branch-coverage cases: Q uniform in [-1, 1], Dirichlet rows for the LEARN players' pi and
        avg, small random update counts (rows 0 stay what creation gave them).  Returns what WolfPopulation.load takes."""
        n, nS = self.n, self.nS
        self.Q_a[:, 1:] = rng.uniform(-1.0, 1.0, (n, nS - 1, 5)); self.Q_b[:, 1:] = rng.uniform(-1.0, 1.0, (n, nS - 1, 5))
        for p in (0, 1):
            if self.learns(p):
                self.pi[p][:, 1:] = rng.dirichlet(np.ones(5), (n, nS - 1)); self.avg[p][:, 1:] = rng.dirichlet(np.ones(5), (n, nS - 1))
        self.updates[:, 1:] = rng.integers(0, max_updates, (n, nS - 1)).astype(np.uint64)
        out = {k: v.copy() for k, v in self.state().items() if k in ROWS + ("updates",)}
        return out

    def state(self, first=0, count=None):
        sl = slice(first, None if count is None else first + count)
        return {"Q_a": self.Q_a[sl], "Q_b": self.Q_b[sl], "pi_a": self.pi[0][sl], "pi_b": self.pi[1][sl], "avg_a": self.avg[0][sl],
                "avg_b": self.avg[1][sl], "updates": self.updates[sl], "alpha": self.alpha[sl], "dscale": self.dscale[sl], "steps": self.steps}


def assert_wolf_population_equal(got, want):
    """bit for bit: a population's read() against another's, or against WolfPopulationNumpy.state()"""
    for k in ROWS + ("alpha", "dscale"):
        g = np.ascontiguousarray(got[k], np.float64).view(np.uint64).reshape(-1)
        w = np.ascontiguousarray(want[k], np.float64).view(np.uint64).reshape(-1)
        assert g.shape == w.shape, (k, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s differs in %d entries, first at flat index %d: %r vs %r" % (
            k, bad.size, bad[0], np.asarray(got[k]).reshape(-1)[bad[0]], np.asarray(want[k]).reshape(-1)[bad[0]])
    np.testing.assert_array_equal(np.asarray(got["updates"], np.uint64), np.asarray(want["updates"], np.uint64), "updates")
    assert int(got["steps"]) == int(want["steps"])
