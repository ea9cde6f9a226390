"""The batched minimax-Q learner of include/soccer_hip.h ("learners") restated in numpy, step for step: the oracle is the
environment (sample_actions_mixed + step on an auto-reset Oracle), the host build of csrc/soccer_games.hpp solves the
stage games (the device build returns the same bits), everything else is the definition's float64 / int64 arithmetic.
tests/test_gpu_minimax_q.py holds the device to it bit for bit; tests/test_minimax_q_np.py checks that it learns.

Also here: shapley_lists / shapley_vi, minimax value iteration on the oracle's transition lists with the same solver —
the V* a learner should approach, computed without the library."""
import numpy as np

from q_learning_np import run_learner
from test_matrix_game_host import solve_host

SCALE = 2.0 ** 40


def thresholds(probs):
    """SoccerBatch.mixed_policy_thresholds, spelled out (this file must not need the library)."""
    c = np.cumsum(np.asarray(probs, np.float64), axis=1)[:, :4]
    return np.ascontiguousarray(np.clip(np.floor(c * 32768.0 + 1e-9), 0, 32768).astype(np.uint16))


def behaviour(pi, explor):
    return thresholds((1.0 - explor) * pi + explor / 5.0)


class MinimaxQNumpy:
    def __init__(self, L, nS, discount_factor, alpha=1.0, decay=0.01 ** (1 / 1e6), explor=0.2, q_init=1.0, opponent="uniform"):
        self.L, self.nS = L, int(nS)
        self.gamma, self.alpha, self.decay, self.explor = float(discount_factor), float(alpha), float(decay), float(explor)
        self.Q = np.full((nS, 5, 5), float(q_init)); self.Q[0] = 0.0
        self.V = np.full(nS, float(q_init)); self.V[0] = 0.0
        self.pi_a = np.full((nS, 5), 0.2); self.pi_b = np.full((nS, 5), 0.2)
        self.visits = np.zeros((nS, 25), np.uint64)
        self.steps = 0
        self.n_truncated = self.n_terminated = self.n_left_out = 0     # what run() met (q_learning_np.run_learner)
        self.opponent = opponent
        self.fixed = None if isinstance(opponent, str) else thresholds(opponent)

    def tables(self):
        """step 1: the threshold tables of the two behaviour policies (mix_b None: uniform)"""
        ma = behaviour(self.pi_a, self.explor)
        if isinstance(self.opponent, str):
            mb = None if self.opponent == "uniform" else behaviour(self.pi_b, self.explor)
        else:
            mb = self.fixed
        return ma, mb

    def update(self, obs, act_a, act_b, reward, terminated, next_obs):
        """steps 3-6 on a batch of transitions (all of them valid)"""
        nS = self.nS
        obs = np.asarray(obs).astype(np.int64); nxt = np.asarray(next_obs).astype(np.int64)
        cell = obs * 25 + np.asarray(act_a).astype(np.int64) * 5 + np.asarray(act_b).astype(np.int64)
        live = 1 - (np.asarray(terminated) != 0).astype(np.int64)
        Vq = np.rint(self.V * SCALE).astype(np.int64)
        c = np.bincount(cell, minlength=nS * 25).astype(np.int64)
        R = np.zeros(nS * 25, np.int64); np.add.at(R, cell, np.asarray(reward).astype(np.int64))
        SV = np.zeros(nS * 25, np.int64); np.add.at(SV, cell, Vq[nxt] * live)
        touched = np.flatnonzero(c)
        if touched.size:
            m = (R[touched].astype(np.float64) + self.gamma * (SV[touched].astype(np.float64) * 2.0 ** -40)) / c[touched].astype(np.float64)
            Qf = self.Q.reshape(-1)
            Qf[touched] = Qf[touched] + self.alpha * (m - Qf[touched])
            self.visits.reshape(-1)[touched] += c[touched].astype(np.uint64)
            ts = np.unique(touched // 25)
            v, x, y, _ = solve_host(self.L, self.Q[ts])
            self.V[ts] = v; self.pi_a[ts] = x; self.pi_b[ts] = y
        self.alpha = self.alpha * self.decay
        self.steps += 1

    def run(self, orc, obs, n_steps):
        """n_steps learner steps on the oracle `orc` whose lanes currently show `obs`; returns the lanes' new observations"""
        return run_learner(self, orc, obs, n_steps)

    def state(self):
        return {"Q": self.Q, "V": self.V, "pi_a": self.pi_a, "pi_b": self.pi_b, "visits": self.visits,
                "alpha": self.alpha, "steps": self.steps}


def assert_learner_equal(got, want):
    """bit for bit: a learner's read() against another's, or against MinimaxQNumpy.state()"""
    for k in ("Q", "V", "pi_a", "pi_b"):
        g = np.ascontiguousarray(got[k], np.float64).view(np.uint64); w = np.ascontiguousarray(want[k], np.float64).view(np.uint64)
        bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
        assert bad.size == 0, "%s differs in %d entries, first at flat index %d: %r vs %r" % (
            k, bad.size, bad[0], np.asarray(got[k]).reshape(-1)[bad[0]], np.asarray(want[k]).reshape(-1)[bad[0]])
    np.testing.assert_array_equal(np.asarray(got["visits"], np.uint64), np.asarray(want["visits"], np.uint64))
    assert np.float64(got["alpha"]).view(np.uint64) == np.float64(want["alpha"]).view(np.uint64), (got["alpha"], want["alpha"])
    assert int(got["steps"]) == int(want["steps"])


def shapley_lists(orc):
    """the two-player P[s][(a, b)] from the oracle's transition relation as padded arrays [nS, 25, K]:
    prob, next observation, player A's reward, 1 - done"""
    lut, kind, gv, isd, isdp = orc.tables()
    W, H, nS = orc.W, orc.H, orc.nS
    ent = [[[] for _ in range(25)] for _ in range(nS)]
    for f in np.flatnonzero(kind == 1).tolist():
        p_ = f & 1; r = f >> 1
        yb = r % W; r //= W; xb = r % H; r //= H; ya = r % W; xa = r // W
        s = int(lut[f])
        for ab in range(25):
            ps, ns, rs, ds = orc.transitions((xa, ya, xb, yb, p_), ab // 5, ab % 5)
            for k in range(len(ps)):
                nf = ((((int(ns[k][0]) * W + int(ns[k][1])) * H + int(ns[k][2])) * W + int(ns[k][3])) << 1) | int(ns[k][4])
                ent[s][ab].append((ps[k], 0 if kind[nf] == 2 else int(lut[nf]), float(rs[k]), bool(ds[k])))
    K = max(len(e) for row in ent for e in row)
    Pp = np.zeros((nS, 25, K)); Pn = np.zeros((nS, 25, K), np.int64); Pr = np.zeros((nS, 25, K)); Pd = np.zeros((nS, 25, K))
    for s in range(nS):
        for ab in range(25):
            for k, (p, nx, r, d) in enumerate(ent[s][ab]):
                Pp[s, ab, k] = p; Pn[s, ab, k] = nx; Pr[s, ab, k] = r; Pd[s, ab, k] = 0.0 if d else 1.0
    return Pp, Pn, Pr, Pd


def shapley_vi(L, lists, gamma, theta=1e-10, max_sweeps=2000):
    Pp, Pn, Pr, Pd = lists
    nS = Pp.shape[0]
    V = np.zeros(nS)
    for _ in range(max_sweeps):
        Q = (Pp * (Pr + gamma * V[Pn] * Pd)).sum(2).reshape(nS, 5, 5)
        v, x, y, _ = solve_host(L, Q); v[0] = 0.0
        d = np.abs(v - V).max(); V = v
        if d < theta:
            return V, Q
    raise AssertionError("Shapley iteration did not converge")
