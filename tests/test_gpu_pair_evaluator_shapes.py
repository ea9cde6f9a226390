"""The pair evaluators on the device (soccer_match_outcomes, soccer_occupancy, soccer_policy_gradient) on every shape of pitch, each
bit for bit against its numpy restatement over the CPU oracle's transition relation (tests/match_outcomes_np.py,
tests/occupancy_np.py, tests/policy_gradient_np.py over minimax_q_np.shapley_lists): the eight pitches of
tests/test_gpu_two_player_shapes.py — an even width (6x4, 6x5), a pitch taller than wide (5x9), slip 0 on a small and on a large
pitch, slip 1, 11x7, and 13x8 with its 21 425 states.  The in-lists under the occupancy and the policy gradient are
csrc/soccer_inlists.hpp's from build_minimax's out-lists, the restatement's come from the oracle: 344 entries at the longest with
an ordinary slip, 152 at slip 1, 40 at slip 0.  The number of states modulo 64, which the transposes of the values meet as a
ragged tile, is 57, 17, 13, 13, 57, 17, 57 and 49; the kick-off states are 4 on the even heights and 2 on the odd ones.

Each pitch's lists, inputs, references and handle are built once for the module (tests/pair_evaluator_cases.py); the restatement
is what takes the time (DESIGN section 23 has the module's wall time), the device part of every test is a few seconds at most.
On 13x8 too the restatement solves all six pairs of the 2 x 3 matrix, about a third of the module's time."""
import os
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_evaluator_cases as pc  # noqa: E402
import policy_gradient_np as pgn  # noqa: E402
from test_gpu_best_response import same_bits  # noqa: E402
from test_gpu_cross_play import kickoff_states  # noqa: E402
from test_gpu_occupancy import features_of  # noqa: E402
from test_gpu_policy_gradient import PAIR_KEYS, SUM_KEYS  # noqa: E402
from test_gpu_two_player_shapes import PITCHES, discount  # noqa: E402

pytestmark = pytest.mark.gpu

THETA = pc.THETA
IDS = pc.IDS
MATCH_KEYS = ("win_a", "win_b", "length", "iterations", "values")
OCCUPANCY_KEYS = ("length", "expect", "iterations", "occupancy")


class Game:
    """one pitch: the cases' lists, matrix and references, and a handle"""

    def __init__(self, w, h, slip):
        self.case = pc.shape(w, h, slip)
        self.batch = SoccerBatch(1, w, h, slip)
        self.got = {}

    def device(self, name, call):
        if name not in self.got:
            self.got[name] = call()
        return self.got[name]

    def gradient(self):
        c = self.case
        return self.device("gradient", lambda: self.batch.policy_gradient(c.A, c.B, THETA, c.c, w_a=pc.W_A, w_b=pc.W_B, normalize=True, values=True))

    def occupancy(self):
        c = self.case
        return self.device("occupancy", lambda: self.batch.occupancy(c.A, c.B, THETA, c.c, features=c.F, values=True))


@pytest.fixture(scope="module")
def game():
    """(w, h, slip) -> Game, built once for this module; afterwards the handles are closed and the lists dropped"""
    games = {}

    def get(w, h, slip):
        if (w, h, slip) not in games:
            games[(w, h, slip)] = Game(w, h, slip)
        return games[(w, h, slip)]

    yield get
    for g in games.values():
        g.batch.close()
    games.clear()
    pc.forget_shapes()


def against(g, got, want, keys, what):
    """the device's arrays against the restatement's"""
    for k in keys:
        same_bits(got[k], want[k], "%s of %s on %dx%d" % (k, what, g.case.w, g.case.h))


def test_the_cases_are_the_two_player_shapes_own():
    assert pc.PITCHES == PITCHES and all(pc.discount(w, h) == discount(w, h) for w, h, _ in PITCHES)
    same_bits(pc.features_of(761), features_of(761), "the features")


@pytest.mark.parametrize("w,h,slip", PITCHES, ids=IDS)
def test_the_handle_is_the_oracle_s_pitch(w, h, slip, game):
    g = game(w, h, slip)
    c = g.case
    assert g.batch.nS == c.nS == pc.n_states(w, h)
    assert kickoff_states(g.batch) == c.starts and len(c.starts) == pc.kickoffs(h)
    assert (c.longest_in_list(), c.lists[0].shape[2]) == pc.IN_LISTS[(w, h, slip)]


@pytest.mark.parametrize("w,h,slip", PITCHES, ids=IDS)
def test_match_outcomes(w, h, slip, game):
    g = game(w, h, slip)
    c = g.case
    want = c.restated()["match"]
    got = g.batch.match_outcomes(c.A, c.B, THETA, c.c, values=True)
    print("%dx%d slip %.1f c %.1f: 2 x 3 match outcomes, sweeps %s" % (w, h, slip, c.c, got["iterations"].tolist()))
    against(g, got, want, MATCH_KEYS, "match outcomes")
    assert (want["iterations"] > 16).any() and want["iterations"].max() <= (220 if c.c == 0.9 else 36)
    assert got["values"].shape == (2, 3, 3, c.nS) and (got["values"][:, :, :, 0] == 0).all() and not np.signbit(got["values"][:, :, :, 0]).any()
    bare = g.batch.match_outcomes(c.A, c.B, THETA, c.c)
    for k in MATCH_KEYS[:4]:
        same_bits(bare[k], got[k], k + " without values")


@pytest.mark.parametrize("w,h,slip", PITCHES, ids=IDS)
def test_occupancy(w, h, slip, game):
    g = game(w, h, slip)
    c = g.case
    want = c.restated()["occupancy"]
    got = g.occupancy()
    print("%dx%d slip %.1f c %.1f: 2 x 3 occupancy, sweeps %s" % (w, h, slip, c.c, got["iterations"].tolist()))
    against(g, got, want, OCCUPANCY_KEYS, "occupancy")
    assert (want["iterations"] > 16).any() and want["iterations"].max() <= (220 if c.c == 0.9 else 36)
    D = got["occupancy"]
    assert D.shape == (2, 3, c.nS) and (D[:, :, 0] == 0).all() and not np.signbit(D[:, :, 0]).any()
    assert (D[:, :, c.starts] >= 1.0 / len(c.starts)).all()     # every kick-off state holds its share of mu at the least
    bare = g.batch.occupancy(c.A, c.B, THETA, c.c, features=c.F)
    for k in OCCUPANCY_KEYS[:3]:
        same_bits(bare[k], got[k], k + " without values")


@pytest.mark.parametrize("w,h,slip", PITCHES, ids=IDS)
def test_policy_gradient(w, h, slip, game):
    g = game(w, h, slip)
    c = g.case
    want = c.restated()["gradient"]
    got = g.gradient()
    it = got["iterations"]
    print("%dx%d slip %.1f gamma %.1f: 2 x 3 policy gradient, V sweeps %s, D sweeps %s" % (w, h, slip, c.c, it[..., 0].tolist(), it[..., 1].tolist()))
    assert sorted(got) == sorted(PAIR_KEYS + SUM_KEYS)
    against(g, got, want, PAIR_KEYS + SUM_KEYS, "the policy gradient")
    for k, s in zip(SUM_KEYS, pgn.reduce(got["occupancy"], got["q_a"], got["q_b"], pc.W_A, pc.W_B, True)):
        same_bits(got[k], s, "%s from the returned pairs" % k)
    # D needs more than one batch of sweeps between synchronisations; V not everywhere (the one-hot pair without slip)
    assert (want["iterations"][..., 1] > 16).any()
    assert want["iterations"].max() <= (220 if c.c == 0.9 else 36)
    D = got["occupancy"]
    assert (D[:, :, 0] == 0).all() and not np.signbit(D[:, :, 0]).any()
    assert (got["q_a"][:, :, 0] == 0).all() and (got["q_b"][:, :, 0] == 0).all() and (got["grad_a"][:, 0] == 0).all()
    assert np.isfinite(got["grad_a"]).all() and np.isfinite(got["grad_b"]).all() and (np.abs(got["grad_a"]) > 1e-3).any()
    bare = g.batch.policy_gradient(c.A, c.B, THETA, c.c, w_a=pc.W_A, w_b=pc.W_B, normalize=True)
    assert sorted(bare) == sorted(("payoff", "iterations") + SUM_KEYS)
    for k in bare:
        same_bits(bare[k], got[k], k + " without values")


@pytest.mark.parametrize("w,h,slip", PITCHES, ids=IDS)
def test_the_policy_gradient_carries_its_siblings_bits(w, h, slip, game):
    g = game(w, h, slip)
    c = g.case
    got = g.gradient()
    payoff, it, V = g.batch.cross_play(c.A, c.B, THETA, c.c, values=True)
    occ = g.occupancy()
    same_bits(got["payoff"], payoff, "payoff against cross_play's"); same_bits(got["V"], V, "V against cross_play's")
    same_bits(got["occupancy"], occ["occupancy"], "occupancy against occupancy's")
    same_bits(got["iterations"], np.stack([it, occ["iterations"]], -1), "iterations against the siblings'")
