"""The batched independent Q-learners of include/soccer_hip.h ("learners, independent Q") restated in numpy, step for step:
the oracle is the environment (sample_actions_mixed + step on an auto-reset Oracle), everything else is the definition's
float64 / int64 arithmetic.  It needs neither the library nor the stage-game solver.  tests/test_gpu_q_learning.py holds the
device to it bit for bit; tests/test_q_learning_np.py checks that it learns."""
import numpy as np

SCALE = 2.0 ** 40


def thresholds(probs):
    """SoccerBatch.mixed_policy_thresholds, spelled out (this file must not need the library)."""
    c = np.cumsum(np.asarray(probs, np.float64), axis=1)[:, :4]
    return np.ascontiguousarray(np.clip(np.floor(c * 32768.0 + 1e-9), 0, 32768).astype(np.uint16))


def behaviour(pi, explor):
    return thresholds((1.0 - explor) * pi + explor / 5.0)


def greedy(Q):
    """one-hot [nS, 5] of the first action that attains max_k Q[s][k]"""
    return np.eye(5)[np.asarray(Q).argmax(1)]


def observations(orc):
    """every lane's observation from the oracle's state and tables(): lut[flat tuple], 0 where the tuple is a goal tuple
    (kind == 2: the terminal observation).  What a lane shows after Oracle.set_state, which returns nothing."""
    lut, kind = orc.tables()[:2]
    W, H = orc.W, orc.H
    f = ((((orc.row_a.astype(np.int64) * W + orc.col_a) * H + orc.row_b) * W + orc.col_b) << 1) | (orc.poss & 1)
    return np.where(kind[f] == 2, 0, lut[f]).astype(np.uint16)


def run_learner(q, orc, obs, n_steps):
    """the learner step of include/soccer_hip.h on the oracle, n_steps times, for any restatement `q` with tables() and
    update(): a lane contributes nothing if it needed reset before the step ("lanes that still need their first reset ...
    contribute nothing") or if its current observation is 0 ("index 0 ... never a current state").  With no such lane every
    transition goes to update() as it is.  Counts into q.n_left_out and, over the transitions it accepted, q.n_terminated and
    q.n_truncated (the flags as the environment sets them, so one transition may count in both; a truncated transition that is
    not terminated is the one after which the lane auto-resets and the learner still bootstraps, from final_obs)."""
    obs = np.asarray(obs).astype(np.uint16)
    for _ in range(int(n_steps)):
        ma, mb = q.tables()
        keep = (((orc.poss >> 1) & 1) == 0) & (obs != 0)
        a, b = orc.sample_actions_mixed(obs, ma, mb)
        out = orc.step(a, b)
        term = out["terminated"][keep] != 0
        q.n_left_out += int(keep.size - keep.sum())
        q.n_terminated += int(term.sum())
        q.n_truncated += int((out["truncated"][keep] != 0).sum())
        q.update(obs[keep], a[keep], b[keep], out["reward"][keep], out["terminated"][keep], out["final_obs"][keep])
        obs = out["obs"]
    return obs


class QLearningNumpy:
    """act_a / act_b: 'greedy' (epsilon-greedy on the player's own table), 'uniform' (the null row table) or a fixed [nS, 5]
    mixed policy.  Q_b is in player B's own reward.  Both tables are always updated."""

    def __init__(self, nS, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, act_a="greedy", act_b="greedy"):
        self.nS = int(nS)
        self.gamma, self.alpha, self.decay, self.explor = float(discount_factor), float(alpha), float(decay), float(explor)
        self.Q_a = np.full((nS, 5), float(q_init)); self.Q_a[0] = 0.0
        self.Q_b = self.Q_a.copy()
        self.visits = np.zeros((nS, 25), np.uint64)
        self.steps = 0
        self.n_truncated = self.n_terminated = self.n_left_out = 0     # what run() met (run_learner)
        self.act = (act_a, act_b)
        self.fixed = tuple(None if isinstance(x, str) else thresholds(x) for x in self.act)

    def _table(self, p):
        if not isinstance(self.act[p], str):
            return self.fixed[p]
        if self.act[p] == "uniform":
            return None
        return behaviour(greedy((self.Q_a, self.Q_b)[p]), self.explor)

    def tables(self):
        """step 1: the threshold tables of the two behaviour policies (None: the null row table)"""
        return self._table(0), self._table(1)

    def update(self, obs, act_a, act_b, reward, terminated, next_obs):
        """steps 3-6 on a batch of transitions (all of them valid)"""
        nS = self.nS
        obs = np.asarray(obs).astype(np.int64); nxt = np.asarray(next_obs).astype(np.int64)
        cell = obs * 25 + np.asarray(act_a).astype(np.int64) * 5 + np.asarray(act_b).astype(np.int64)
        live = 1 - (np.asarray(terminated) != 0).astype(np.int64)
        Vq_a = np.rint(self.Q_a.max(1) * SCALE).astype(np.int64)
        Vq_b = np.rint(self.Q_b.max(1) * SCALE).astype(np.int64)
        c = np.bincount(cell, minlength=nS * 25).astype(np.int64).reshape(nS, 5, 5)
        R = np.zeros(nS * 25, np.int64); np.add.at(R, cell, np.asarray(reward).astype(np.int64))
        SA = np.zeros(nS * 25, np.int64); np.add.at(SA, cell, Vq_a[nxt] * live)
        SB = np.zeros(nS * 25, np.int64); np.add.at(SB, cell, Vq_b[nxt] * live)
        R = R.reshape(nS, 5, 5); SA = SA.reshape(nS, 5, 5); SB = SB.reshape(nS, 5, 5)
        # player A sums over b, player B over a and in its own reward
        for Q, cc, RR, SV in ((self.Q_a, c.sum(2), R.sum(2), SA.sum(2)), (self.Q_b, c.sum(1), -R.sum(1), SB.sum(1))):
            t = cc > 0
            m = (RR[t].astype(np.float64) + self.gamma * (SV[t].astype(np.float64) * 2.0 ** -40)) / cc[t].astype(np.float64)
            Q[t] = Q[t] + self.alpha * (m - Q[t])
        self.visits += c.reshape(nS, 25).astype(np.uint64)
        self.alpha = self.alpha * self.decay
        self.steps += 1

    def run(self, orc, obs, n_steps):
        """n_steps learner steps on the oracle `orc` whose lanes currently show `obs`; returns the lanes' new observations"""
        return run_learner(self, orc, obs, n_steps)

    def state(self):
        return {"Q_a": self.Q_a, "Q_b": self.Q_b, "V_a": self.Q_a.max(1), "V_b": self.Q_b.max(1), "pi_a": greedy(self.Q_a),
                "pi_b": greedy(self.Q_b), "visits": self.visits, "alpha": self.alpha, "steps": self.steps}


def assert_learner_equal(got, want):
    """bit for bit: a learner's read() against another's, or against QLearningNumpy.state()"""
    for k in ("Q_a", "Q_b", "V_a", "V_b", "pi_a", "pi_b"):
        g = np.ascontiguousarray(got[k], np.float64).view(np.uint64); w = np.ascontiguousarray(want[k], np.float64).view(np.uint64)
        bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
        assert bad.size == 0, "%s differs in %d entries, first at flat index %d: %r vs %r" % (
            k, bad.size, bad[0], np.asarray(got[k]).reshape(-1)[bad[0]], np.asarray(want[k]).reshape(-1)[bad[0]])
    np.testing.assert_array_equal(np.asarray(got["visits"], np.uint64), np.asarray(want["visits"], np.uint64))
    assert np.float64(got["alpha"]).view(np.uint64) == np.float64(want["alpha"]).view(np.uint64), (got["alpha"], want["alpha"])
    assert int(got["steps"]) == int(want["steps"])
