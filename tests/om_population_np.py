"""The population of opponent-modelling Q-learners of include/soccer_hip.h ("learners, a population of opponent-modelling
Q-learners") restated in numpy, vectorised over the members: per player a joint-action table [n, nS, 5, 5] (own action, the
other's action) and the counts [n, nS, 5] of the other player's actions, member i fed by lane i of the oracle alone.  The
oracle is the environment, as for tests/q_population_np.py (n <= 65 535).  tests/test_om_population_np.py holds it to n
separate scalar-loop learners written from the header's text, bit for bit, and checks that it learns;
tests/test_gpu_om_population.py holds the device to it bit for bit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from q_learning_np import SCALE, thresholds  # noqa: E402


def derive(Q, C):
    """THE derived values, by the header's expression: Q [..., 5, 5], C [..., 5] uint64 -> (V [...], g [...]).  Every product and
    every sum is one numpy operation, so each is rounded on its own, in the header's order."""
    Q = np.asarray(Q, np.float64); C = np.asarray(C, np.uint64)
    n = C[..., 0] + C[..., 1] + C[..., 2] + C[..., 3] + C[..., 4]
    seen = n > 0
    w = np.where(seen[..., None], C.astype(np.float64), 1.0)
    N = np.where(seen, n.astype(np.float64), 5.0)
    W = w[..., None, 0] * Q[..., 0]
    for k in range(1, 5):
        W = W + w[..., None, k] * Q[..., k]
    g = W.argmax(-1)                                    # the first index that attains the maximum
    Wg = np.take_along_axis(W, g[..., None], -1)[..., 0]
    return np.minimum(1.0, np.maximum(-1.0, Wg / N)), g


class OMPopulationNumpy:
    """act_a / act_b: 'greedy', 'uniform' or a fixed [nS, 5] mixed policy shared by all members.  discount_factor, alpha, decay
    and explor: scalars, or arrays of n."""

    def __init__(self, n, nS, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, act_a="greedy", act_b="greedy"):
        self.n, self.nS = int(n), int(nS)
        assert self.n <= 65535
        per = lambda x: np.broadcast_to(np.asarray(x, np.float64), (self.n,)).copy()  # noqa: E731
        self.gamma, self.alpha, self.decay, self.explor = per(discount_factor), per(alpha), per(decay), per(explor)
        self.Q_a = np.full((self.n, self.nS, 5, 5), float(q_init)); self.Q_a[:, 0] = 0.0
        self.Q_b = self.Q_a.copy()
        self.C_a = np.zeros((self.n, self.nS, 5), np.uint64); self.C_b = self.C_a.copy()
        self.steps = 0
        self.n_same = self.n_terminated = self.n_truncated_only = self.n_left_out = self.n_first_seen = 0      # what run() met
        self.act = (act_a, act_b)
        self.fixed = tuple(None if isinstance(x, str) else thresholds(x) for x in self.act)
        self.lanes = np.arange(self.n)

    def _derive(self, p, members, s):
        """(V, g) of player p of `members` at their states s"""
        return derive((self.Q_a, self.Q_b)[p][members, s], (self.C_a, self.C_b)[p][members, s])

    def _rows(self, p, obs):
        """step 1 for player p: every member's threshold row at its lane's observation, [n, 4] (None: the null row table)"""
        if self.fixed[p] is not None:
            return self.fixed[p][obs]
        if self.act[p] == "uniform":
            return None
        pi = np.eye(5)[self._derive(p, self.lanes, np.asarray(obs).astype(np.int64))[1]]
        e = self.explor[:, None]
        return thresholds((1.0 - e) * pi + e / 5.0)

    def update(self, obs, act_a, act_b, reward, terminated, next_obs, keep=None):
        """steps 3-6, transition i for member i; members outside `keep` (bool [n]) leave their tables and counts alone, every
        alpha advances"""
        i = self.lanes if keep is None else self.lanes[np.asarray(keep, bool)]
        s = np.asarray(obs).astype(np.int64)[i]; s2 = np.asarray(next_obs).astype(np.int64)[i]
        live = 1 - (np.asarray(terminated)[i] != 0).astype(np.int64)
        r = np.asarray(reward).astype(np.int64)[i]
        a = np.asarray(act_a).astype(np.int64)[i]; b = np.asarray(act_b).astype(np.int64)[i]
        # both bootstraps are read before anything moves (s' may be s)
        sv = [np.rint(self._derive(p, i, s2)[0] * SCALE).astype(np.int64) * live for p in (0, 1)]
        self.n_first_seen += int((self.C_a[i, s].sum(1) == 0).sum())
        for Q, C, own, other, R, SV in ((self.Q_a, self.C_a, a, b, r, sv[0]), (self.Q_b, self.C_b, b, a, -r, sv[1])):
            m = R.astype(np.float64) + self.gamma[i] * (SV.astype(np.float64) * 2.0 ** -40)
            q = Q[i, s, own, other]
            Q[i, s, own, other] = q + self.alpha[i] * (m - q)
            C[i, s, other] += np.uint64(1)
        self.alpha = self.alpha * self.decay
        self.steps += 1

    def run(self, orc, obs, n_steps):
        """n_steps steps of every member on the oracle `orc` (n lanes) whose lanes currently show `obs`; returns the lanes' new
        observations.  A lane contributes nothing if it needed reset before the step or if its observation is 0."""
        obs = np.asarray(obs).astype(np.uint16)
        for _ in range(int(n_steps)):
            keep = (((orc.poss >> 1) & 1) == 0) & (obs != 0)
            a, b = orc.sample_actions_mixed(self.lanes, self._rows(0, obs), self._rows(1, obs))
            out = orc.step(a, b)
            term = out["terminated"] != 0
            self.n_left_out += int(keep.size - keep.sum())
            self.n_same += int((keep & (out["final_obs"] == obs)).sum())
            self.n_terminated += int((keep & term).sum())
            self.n_truncated_only += int((keep & ~term & (out["truncated"] != 0)).sum())
            self.update(obs, a, b, out["reward"], out["terminated"], out["final_obs"], keep)
            obs = out["obs"]
        return obs

    def state(self, first=0, count=None):
        sl = slice(first, None if count is None else first + count)
        return {"Q_a": self.Q_a[sl], "Q_b": self.Q_b[sl], "C_a": self.C_a[sl], "C_b": self.C_b[sl], "alpha": self.alpha[sl],
                "steps": self.steps}


def assert_om_population_equal(got, want):
    """bit for bit: a population's read() against another's, or against OMPopulationNumpy.state()"""
    for k in ("Q_a", "Q_b", "alpha"):
        g = np.ascontiguousarray(got[k], np.float64).view(np.uint64).reshape(-1)
        w = np.ascontiguousarray(want[k], np.float64).view(np.uint64).reshape(-1)
        assert g.shape == w.shape, (k, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s differs in %d entries, first at flat index %d: %r vs %r" % (
            k, bad.size, bad[0], np.asarray(got[k]).reshape(-1)[bad[0]], np.asarray(want[k]).reshape(-1)[bad[0]])
    for k in ("C_a", "C_b"):
        np.testing.assert_array_equal(np.asarray(got[k], np.uint64), np.asarray(want[k], np.uint64), err_msg=k)
    assert int(got["steps"]) == int(want["steps"])
