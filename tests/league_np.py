"""The league opponent of the population of Q-learners (include/soccer_hip.h, "learners, a league opponent for the population
of Q-learners") restated in numpy: QPopulationNumpy plus one word per member, the pick.  The word of a kick-off draw comes
from philox_np (written from the specification, not through oracle/), the league player's rows thr[pick, obs] go to the
oracle's sample_actions_mixed like every other row.  tests/test_league_np.py holds it to QPopulationNumpy where the two must
agree and checks the pick function at its boundaries; tests/test_gpu_league.py holds the device to it bit for bit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from philox_np import lane_words  # noqa: E402
from q_learning_np import thresholds  # noqa: E402
from q_population_np import QPopulationNumpy, assert_population_equal  # noqa: E402


def league_thresholds(weights):
    """T_k = min(2^32, floor(c_k * 2^32)) for k < K - 1 as Python-exact integers in a uint64 array, c_k the sequential float64
    sum w_0 + .. + w_k"""
    w = np.asarray(weights, np.float64)
    T, c = [], 0.0
    for k in range(w.size - 1):
        c = c + float(w[k])
        T.append(min(2 ** 32, int(np.floor(c * 4294967296.0))))
    return np.array(T, np.uint64)


def league_pick(T, words):
    """#{k < K - 1 : W >= T_k} for every word: the definition, counted one threshold at a time"""
    W = np.asarray(words).astype(np.uint64)
    pick = np.zeros(W.shape, np.int32)
    for t in np.asarray(T, np.uint64):
        pick += (W >= t).astype(np.int32)
    return pick


class QLeagueNumpy(QPopulationNumpy):
    """league_player 0 / 1 plays policies [K, nS, 5] with weights [K]; `other` is how the other player acts ('greedy',
    'uniform' or a fixed [nS, 5] policy).  The remaining arguments are QPopulationNumpy's."""

    def __init__(self, n, nS, discount_factor, league_player, policies, weights, other="greedy", **kw):
        acts = {"act_a": "uniform", "act_b": other} if league_player == 0 else {"act_a": other, "act_b": "uniform"}   # (a placeholder)
        super().__init__(n, nS, discount_factor, **acts, **kw)
        self.league = int(league_player)
        pol = np.asarray(policies, np.float64)
        self.K = pol.shape[0]
        self.thr = np.stack([thresholds(p) for p in pol])          # [K, nS, 4], the fixed policies' own expression
        self.T = league_thresholds(weights)
        self.pick = np.full(self.n, -1, np.int32)
        self.n_redraws = 0              # draws after the first: a finished episode, or a loaded -1
        self.max_live = 0               # the most different picks live at one step
        self.seen = set()               # every pick that was ever live
        self._drawn = np.zeros(self.n, bool)

    def _rows(self, p, obs):
        if p == self.league:
            return self.thr[self.pick, obs]
        return super()._rows(p, obs)

    def run(self, orc, obs, n_steps):
        obs = np.asarray(obs).astype(np.uint16)
        for _ in range(int(n_steps)):
            need = self.pick < 0                                    # frozen and parked lanes draw too
            if need.any():
                W = lane_words(orc.seed, orc.lane_offset + self.lanes, 2 ** 62 + orc.tick, purpose=1)
                self.pick = np.where(need, league_pick(self.T, W), self.pick).astype(np.int32)
                self.n_redraws += int((need & self._drawn).sum())
                self._drawn |= need
            self.max_live = max(self.max_live, np.unique(self.pick).size)
            self.seen |= set(self.pick.tolist())
            keep = (((orc.poss >> 1) & 1) == 0) & (obs != 0)
            frozen = ((orc.poss >> 1) & 1) != 0
            a, b = orc.sample_actions_mixed(self.lanes, self._rows(0, obs), self._rows(1, obs))
            out = orc.step(a, b)
            term = out["terminated"] != 0
            self.n_left_out += int(keep.size - keep.sum())
            self.n_same += int((keep & (out["final_obs"] == obs)).sum())
            self.n_terminated += int((keep & term).sum())
            self.n_truncated_only += int((keep & ~term & (out["truncated"] != 0)).sum())
            self.update(obs, a, b, out["reward"], out["terminated"], out["final_obs"], keep)
            finished = ~frozen & (term | (out["truncated"] != 0))   # a frozen lane is left untouched: nothing finished
            self.pick = np.where(finished, -1, self.pick).astype(np.int32)
            obs = out["obs"]
        return obs

    def state(self, first=0, count=None):
        s = super().state(first, count)
        s["pick"] = self.pick[slice(first, None if count is None else first + count)]
        return s


def assert_league_equal(got, want):
    """assert_population_equal and the picks"""
    assert_population_equal(got, want)
    np.testing.assert_array_equal(np.asarray(got["pick"], np.int32), np.asarray(want["pick"], np.int32))
