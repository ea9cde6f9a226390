"""The two-player solvers on the device (soccer_minimax_value_iteration / soccer_minimax_backup, soccer_best_response,
soccer_evaluate_policies, soccer_cross_play) on every shape of pitch, each bit for bit against its numpy restatement over the
CPU oracle's transition relation (tests/minimax_vi_np.py, tests/best_response_np.py, tests/cross_play_np.py over
minimax_q_np.shapley_lists): an even width (6x4, 6x5), a pitch taller than wide (5x9), slip 0 and slip 1, 8x7 and 11x7, and 13x8,
which is above the 19 013 states of 14x7 where the single-agent planners stop — these solvers keep V in global memory and
accept it.  The lists under every solve are build_minimax's (enumerate_kernel, minimax_lists_kernel, tuple_of, the padding to
kPlanPad); the restatement's come from the oracle, so a list built in another order, another padding, another stopping sweep or
another buffer parity shows here on the pitch where it bites.

Each pitch's lists, inputs, references and handle are built once for the module; the restatement is what takes the time
(DESIGN section 9 has the module's wall time), the device part of every test is a few seconds at most."""
import os
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch
from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_response_np as brn  # noqa: E402
import cross_play_np as cpn  # noqa: E402
import minimax_vi_np as mvn  # noqa: E402
from minimax_q_np import shapley_lists  # noqa: E402
from test_gpu_best_response import same_bits  # noqa: E402
from test_gpu_cross_play import kickoff_states  # noqa: E402
from test_matrix_game_host import assert_certificate, build_games_host  # noqa: E402

pytestmark = pytest.mark.gpu

THETA = 1e-10
# width, height, slip
PITCHES = [(5, 4, 0.0), (6, 4, 0.2), (6, 5, 0.2), (7, 5, 1.0), (5, 9, 0.3), (8, 7, 0.0), (11, 7, 0.2), (13, 8, 0.1)]
IDS = ["%dx%d" % p[:2] for p in PITCHES]
PLANNERS_LARGEST = (14, 7)                                      # the last pitch the single-agent planners accept


def n_states(w, h):
    return 2 * w * h * (w * h - 1) + 1


def discount(w, h):
    """0.9 up to 7x5, 0.5 on the larger pitches: about 30 sweeps of the restatement instead of about 200"""
    return 0.9 if n_states(w, h) <= n_states(7, 5) else 0.5


class Game:
    """one pitch: the oracle, its two-player lists, the inputs of every test and a handle, built once"""

    def __init__(self, w, h, slip, host):
        self.w, self.h, self.slip, self.host = w, h, slip, host
        self.gamma = discount(w, h)
        self.orc = Oracle(w, h, slip, n=1, seed=0)
        self.nS = self.orc.nS
        self.lists = shapley_lists(self.orc)
        self.starts = cpn.isd_obs(self.orc)
        rng = np.random.default_rng(w * 100 + h)
        self.V = rng.uniform(-1, 1, self.nS)                    # the backup's input
        nS = self.nS
        # best_response and evaluate_policies: a Dirichlet(0.2) policy and a one-hot policy
        self.pol = np.stack([rng.dirichlet(np.full(5, 0.2), nS), brn.onehot(rng.integers(0, 5, nS))])
        # cross-play, 2 x 3: pair (0, 1) of the matrix is the pair evaluate_policies gets
        self.A = self.pol
        self.B = np.stack([np.full((nS, 5), 0.2), self.pol[1], rng.dirichlet(np.ones(5), nS)])
        self.batch = SoccerBatch(1, w, h, slip)
        self.ref = {}

    def want(self, name, call):
        """a result of the restatement, computed once"""
        if name not in self.ref:
            self.ref[name] = call()
        return self.ref[name]

    def cross(self):
        return self.want("cross", lambda: cpn.cross_play(self.lists, self.starts, self.A, self.B, self.gamma, THETA))


@pytest.fixture(scope="module")
def game(tmp_path_factory):
    """(w, h, slip) -> Game, built once for this module; afterwards the handles are closed and the lists dropped"""
    host = build_games_host(tmp_path_factory.mktemp("games_shapes"))
    games = {}

    def get(w, h, slip):
        if (w, h, slip) not in games:
            games[(w, h, slip)] = Game(w, h, slip, host)
        return games[(w, h, slip)]

    yield get
    for g in games.values():
        g.batch.close()
    games.clear()


def test_the_pitches_sit_where_they_should():
    sizes = [p[:2] for p in PITCHES]
    nS = [n_states(w, h) for w, h in sizes]
    assert len(set(PITCHES)) == len(PITCHES)
    assert any(w % 2 == 0 and n < n_states(7, 5) for (w, h), n in zip(sizes, nS)) and (6, 4) in sizes      # an even width
    assert any(h > w for w, h in sizes) and (5, 9) in sizes                                                # taller than wide
    assert {0.0, 1.0} <= {p[2] for p in PITCHES} and any(0.0 < p[2] < 1.0 for p in PITCHES)
    assert (8, 7) in sizes and (11, 7) in sizes
    assert max(nS) > n_states(*PLANNERS_LARGEST) == 19013 and n_states(13, 8) == 21425 and (13, 8) in sizes
    assert max(nS) <= 65535                                     # the uint16 observation index
    # nS = 2 n (n - 1) + 1 is 1 mod 4: the two residues mod 8 (the lists are read kPlanPad = 4 entries at a time, the sweeps
    # take 4 and 8 states a workgroup), and cross_values_kernel's 64 x 64 tile ragged in three different ways
    assert all(n % 4 == 1 for n in nS) and {n % 8 for n in nS} == {1, 5}
    assert len({n % 64 for n in nS}) >= 3 and 0 not in {n % 64 for n in nS}
    # nS mod 8 = 5 (and mod 64 = 13) both at slip 1 and at an ordinary slip, so a failure there names the slip or the tail
    assert {p[2] for p, n in zip(PITCHES, nS) if n % 8 == 5} == {0.2, 1.0}
    # more than one workgroup of every sweep kernel everywhere, and the discounts
    assert min(nS) > 8 and [discount(w, h) for w, h in sizes] == [0.9, 0.9, 0.9, 0.9, 0.5, 0.5, 0.5, 0.5]


@pytest.mark.parametrize("w,h,slip", PITCHES, ids=IDS)
def test_the_handle_is_the_oracle_s_pitch(w, h, slip, game):
    g = game(w, h, slip)
    assert g.batch.nS == g.nS == n_states(w, h)
    assert kickoff_states(g.batch) == g.starts


@pytest.mark.parametrize("w,h,slip", PITCHES, ids=IDS)
def test_minimax_value_iteration(w, h, slip, game):
    g = game(w, h, slip)
    wa, wb, wV, wQ, wk, capped = g.want("vi", lambda: mvn.minimax_vi(g.host, g.lists, g.gamma, THETA))
    assert not capped and wk > 16                               # (more than one batch of sweeps between synchronisations)
    pa, pb, V, Q, k = g.batch.minimax_value_iteration(THETA, g.gamma)
    print("%dx%d slip %.1f gamma %.1f: minimax value iteration, %d sweeps (the restatement: %d)" % (w, h, slip, g.gamma, k, wk))
    assert k == wk
    same_bits(Q, wQ, "Q"); same_bits(V, wV, "V"); same_bits(pa, wa, "pi_a"); same_bits(pb, wb, "pi_b")
    assert_certificate(Q, V, pa, pb)


@pytest.mark.parametrize("w,h,slip", PITCHES, ids=IDS)
def test_one_backup_from_a_random_v(w, h, slip, game):
    g = game(w, h, slip)
    wa, wb, wV, wQ = g.want("backup", lambda: mvn.backup(g.host, g.lists, g.V, g.gamma))
    pa, pb, V, Q, one = g.batch.minimax_backup(g.V, g.gamma)
    assert one == 1
    same_bits(Q, wQ, "Q"); same_bits(V, wV, "V"); same_bits(pa, wa, "pi_a"); same_bits(pb, wb, "pi_b")


@pytest.mark.parametrize("player", [0, 1])
@pytest.mark.parametrize("w,h,slip", PITCHES, ids=IDS)
def test_best_response(w, h, slip, player, game):
    g = game(w, h, slip)
    wbr, wV, wQr, wit = g.want("br%d" % player, lambda: brn.best_response(g.lists, g.pol, player, g.gamma, THETA))
    br, V, Qr, it = g.batch.best_response(g.pol, player, THETA, g.gamma)
    print("%dx%d slip %.1f gamma %.1f: response to player %s's policies, sweeps %s" % (w, h, slip, g.gamma, "AB"[player], it.tolist()))
    same_bits(it, wit, "iterations"); same_bits(Qr, wQr, "Qr"); same_bits(V, wV, "V"); same_bits(br, wbr, "br")
    assert (wit > 16).all()


@pytest.mark.parametrize("w,h,slip", PITCHES, ids=IDS)
def test_evaluate_policies(w, h, slip, game):
    g = game(w, h, slip)
    _, wit, wV = g.cross()                                      # the pair (pol[0], pol[1]) is the matrix's pair (0, 1)
    V, it = g.batch.evaluate_policies(g.pol[0], g.pol[1], THETA, g.gamma)
    assert it == wit[0, 1]
    same_bits(V, wV[0, 1], "V of the pair")


@pytest.mark.parametrize("w,h,slip", PITCHES, ids=IDS)
def test_cross_play(w, h, slip, game):
    g = game(w, h, slip)
    want = g.cross()
    got = g.batch.cross_play(g.A, g.B, THETA, g.gamma, values=True)
    print("%dx%d slip %.1f gamma %.1f: 2 x 3 cross-play, sweeps %s" % (w, h, slip, g.gamma, got[1].tolist()))
    for name, x, y in zip(("iterations", "V", "payoff"), (got[1], got[2], got[0]), (want[1], want[2], want[0])):
        same_bits(x, y, name)
    assert (want[1] > 16).all()                                 # (more than one batch of sweeps between synchronisations)
