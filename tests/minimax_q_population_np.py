"""The population of minimax-Q learners of include/soccer_hip.h ("learners, a population of minimax-Q learners") restated in
numpy, vectorised over the members: Q[n, nS, 5, 5], V[n, nS], pi_a / pi_b [n, nS, 5], member i fed by lane i of the oracle
alone.  The oracle is the environment (as for tests/q_population_np.py); the host build of csrc/soccer_games.hpp solves the
stage games, ONE batched solve_host call per step for all members (the device build returns the same bits); everything else is
the definition's float64 / int64 arithmetic, one elementwise operation at a time.  It counts the solver's return codes.
tests/test_minimax_q_population_np.py holds it to n separate MinimaxQNumpy instances of one lane each bit for bit and checks
that it learns; tests/test_gpu_minimax_q_population.py holds the device to it bit for bit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from q_learning_np import SCALE, thresholds  # noqa: E402
from q_population_np import QPopulationNumpy  # noqa: E402
from test_matrix_game_host import solve_host  # noqa: E402

ROWS = ("Q", "V", "pi_a", "pi_b")


class MinimaxQPopulationNumpy(QPopulationNumpy):
    """opponent: 'uniform', 'self', a fixed [nS, 5] mixed policy for every member or [n, nS, 5], one per member.
    discount_factor, alpha, decay and explor: scalars, or arrays of n.  L: build_games_host's library.  run() is
    QPopulationNumpy's loop."""

    def __init__(self, L, n, nS, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, opponent="uniform"):
        self.L, self.n, self.nS = L, int(n), int(nS)
        assert self.n <= 65535
        per = lambda x: np.broadcast_to(np.asarray(x, np.float64), (self.n,)).copy()  # noqa: E731
        self.gamma, self.alpha, self.decay, self.explor = per(discount_factor), per(alpha), per(decay), per(explor)
        self.Q = np.full((self.n, self.nS, 5, 5), float(q_init)); self.Q[:, 0] = 0.0
        self.V = np.full((self.n, self.nS), float(q_init)); self.V[:, 0] = 0.0
        self.pi_a = np.full((self.n, self.nS, 5), 0.2); self.pi_b = np.full((self.n, self.nS, 5), 0.2)      # set, not solved
        self.steps = 0
        self.n_same = self.n_terminated = self.n_truncated_only = self.n_left_out = 0      # what run() met
        self.codes = np.zeros(4, np.int64)          # solve_game5's return codes: simplex, saddle point, enumeration, none passed
        self.opponent = opponent
        self.fixed = None                           # the host-computed thresholds: [nS, 4] or [n, nS, 4]
        if not isinstance(opponent, str):
            pol = np.asarray(opponent, np.float64)
            self.fixed = thresholds(pol.reshape(-1, 5)).reshape(pol.shape[:-1] + (4,))
        self.lanes = np.arange(self.n)

    def _rows(self, p, obs):
        """step 1 for player p: every member's threshold row at its lane's observation, [n, 4] (None: the null row table)"""
        e = self.explor[:, None]
        if p == 0:
            return thresholds((1.0 - e) * self.pi_a[self.lanes, obs] + e / 5.0)
        if self.fixed is not None:
            return self.fixed[obs] if self.fixed.ndim == 2 else self.fixed[self.lanes, obs]
        if self.opponent == "uniform":
            return None
        return thresholds((1.0 - e) * self.pi_b[self.lanes, obs] + e / 5.0)

    def update(self, obs, act_a, act_b, reward, terminated, next_obs, keep=None):
        """steps 3-6, transition i for member i; members outside `keep` (bool [n]) are left alone, every alpha advances"""
        i = self.lanes if keep is None else self.lanes[np.asarray(keep, bool)]
        s = np.asarray(obs).astype(np.int64)[i]; s2 = np.asarray(next_obs).astype(np.int64)[i]
        a = np.asarray(act_a).astype(np.int64)[i]; b = np.asarray(act_b).astype(np.int64)[i]
        live = 1 - (np.asarray(terminated)[i] != 0).astype(np.int64)
        r = np.asarray(reward).astype(np.int64)[i]
        SV = np.rint(self.V[i, s2] * SCALE).astype(np.int64) * live             # read before the re-solve (s' may be s)
        m = (r.astype(np.float64) + self.gamma[i] * (SV.astype(np.float64) * 2.0 ** -40)) / 1.0
        q = self.Q[i, s, a, b]
        self.Q[i, s, a, b] = q + self.alpha[i] * (m - q)
        if i.size:
            v, x, y, code = solve_host(self.L, self.Q[i, s])
            self.V[i, s] = v; self.pi_a[i, s] = x; self.pi_b[i, s] = y
            self.codes += np.bincount(code, minlength=4)[:4]
        self.alpha = self.alpha * self.decay
        self.steps += 1

    def solve(self, first=0, count=None):
        """what load() of Q alone does: every live state of the range is re-solved"""
        sl = slice(first, None if count is None else first + count)
        Q = self.Q[sl, 1:]
        v, x, y, code = solve_host(self.L, Q.reshape(-1, 5, 5))
        self.V[sl, 1:] = v.reshape(Q.shape[:2]); self.pi_a[sl, 1:] = x.reshape(Q.shape[:2] + (5,)); self.pi_b[sl, 1:] = y.reshape(Q.shape[:2] + (5,))
        return code

    def load(self, rng):
        """the loaded state of the short runs: Q uniform in [-1, 1] on the live states, V and the strategies solved from it (a
        fresh table is constant, so every early stage game would be a saddle point).  Returns what MinimaxQPopulation.load
        takes: Q alone."""
        self.Q[:, 1:] = rng.uniform(-1.0, 1.0, (self.n, self.nS - 1, 5, 5))
        self.solve()
        return {"Q": self.Q.copy()}

    def state(self, first=0, count=None):
        sl = slice(first, None if count is None else first + count)
        return {"Q": self.Q[sl], "V": self.V[sl], "pi_a": self.pi_a[sl], "pi_b": self.pi_b[sl], "alpha": self.alpha[sl], "steps": self.steps}


def assert_minimax_q_population_equal(got, want):
    """bit for bit: a population's read() against another's, or against MinimaxQPopulationNumpy.state()"""
    for k in ROWS + ("alpha",):
        g = np.ascontiguousarray(got[k], np.float64).view(np.uint64).reshape(-1)
        w = np.ascontiguousarray(want[k], np.float64).view(np.uint64).reshape(-1)
        assert g.shape == w.shape, (k, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s differs in %d entries, first at flat index %d: %r vs %r" % (
            k, bad.size, bad[0], np.asarray(got[k]).reshape(-1)[bad[0]], np.asarray(want[k]).reshape(-1)[bad[0]])
    assert int(got["steps"]) == int(want["steps"])
