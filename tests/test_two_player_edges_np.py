"""Where there is no GPU: every case of tests/test_gpu_two_player_edges.py reaches the path it is there for, shown on the numpy
restatements alone (tests/minimax_vi_np.py, tests/best_response_np.py, tests/cross_play_np.py) on 5x4 at slips 0.0 and 0.2 —
the tied optima, both classes of policy under the cap at discount 1, sweep 2 at discount 0, sweep 1 at theta = +inf, the cap
itself at theta = 0, the policy rows that the documented rule accepts and refuses, and the sweep bound of the low-discount
matrix that the library's own pass split is run on.  The cases are those of tests/two_player_cases.py, which the GPU module
imports too, so both see the same inputs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_response_np as brn  # noqa: E402
import cross_play_np as cpn  # noqa: E402
import minimax_vi_np as mvn  # noqa: E402
from test_matrix_game_host import build_games_host  # noqa: E402
from two_player_cases import (GAMMA0_TIED, INF, NS, PASS_GAMMA, PASS_NA, PASS_NB, PASS_PAIRS, PASS_SWEEPS, SLIPS, THETA, THETA0_CAPS,  # noqa: E402
                              TIE_COUNTS, TIE_GAMMAS, UNDISCOUNTED_CAP, boundary_sample, edge_policies, odd_rows, pass_policies, pass_sample,
                              pitch, refused_rows, restated_pairs, row_accepted, tied_states)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_games_host(tmp_path_factory.mktemp("games_edges"))


@pytest.mark.parametrize("slip", SLIPS)
def test_discount_0_stops_at_sweep_2_with_ties_nearly_everywhere(slip, host):
    lists, starts = pitch(slip)
    pol = edge_policies()
    assert mvn.minimax_vi(host, lists, 0.0, THETA)[4:] == (2, False)
    for player in (0, 1):
        br, V, Qr, it = brn.best_response(lists, pol, player, 0.0, THETA)
        assert it.tolist() == [2] * 4
        assert tied_states(Qr, player).tolist() == [GAMMA0_TIED] * 4
        assert (br[:, 1:] == 0).sum() > 4 * 700                 # the first index of a tie is nearly always action 0
    assert brn.evaluate(lists, pol, np.roll(pol, 1, 0), 0.0, THETA)[1].tolist() == [2] * 4
    # (a pair under which nobody ever scores has V_1 = 0 = V_0 and stops at sweep 1: 'always action 2' against itself at slip 0)
    _, it, V = cpn.cross_play(lists, starts, pol, pol, 0.0, THETA)
    assert ((it == 2) | ((it == 1) & (V == 0.0).all(-1))).all() and (it == 2).sum() >= 15


@pytest.mark.parametrize("slip", SLIPS)
def test_discount_1_leaves_both_classes_under_the_cap(slip, host):
    lists, starts = pitch(slip)
    pol = edge_policies()
    for player in (0, 1):
        it = brn.best_response(lists, pol, player, 1.0, THETA, UNDISCOUNTED_CAP)[3]
        print("slip %.1f, response to player %s at discount 1: sweeps %s" % (slip, "AB"[player], it.tolist()))
        assert it[0] == {0.0: 111, 0.2: 159}[slip] and it[1] == UNDISCOUNTED_CAP
    it = cpn.cross_play(lists, starts, pol, pol, 1.0, THETA, UNDISCOUNTED_CAP)[1]
    print("slip %.1f, 4 x 4 cross-play at discount 1: sweeps\n%s" % (slip, it))
    assert (it == UNDISCOUNTED_CAP).any() and (it < UNDISCOUNTED_CAP).any()
    # minimax value iteration itself is still open at the cap, on both slips
    assert mvn.minimax_vi(host, lists, 1.0, THETA, UNDISCOUNTED_CAP)[4:] == (UNDISCOUNTED_CAP, True)


@pytest.mark.parametrize("slip", SLIPS)
def test_theta_inf_stops_at_sweep_1_and_theta_0_never(slip, host):
    lists, starts = pitch(slip)
    pol = edge_policies()
    assert mvn.minimax_vi(host, lists, 0.9, INF)[4:] == (1, False)
    assert brn.best_response(lists, pol, 0, 0.9, INF)[3].tolist() == [1] * 4
    assert brn.evaluate(lists, pol, pol[::-1], 0.9, INF)[1].tolist() == [1] * 4
    # theta = 0: even the solve that has reached its fixed point exactly (discount 0, sweep 2) goes on to the cap
    for cap in (THETA0_CAPS[0], THETA0_CAPS[-1]):
        assert mvn.minimax_vi(host, lists, 0.9, 0.0, cap)[4:] == (cap, True)
        assert brn.best_response(lists, pol, 1, 0.0, 0.0, cap)[3].tolist() == [cap] * 4
        assert brn.evaluate(lists, pol, pol[::-1], 0.9, 0.0, cap)[1].tolist() == [cap] * 4
    assert THETA0_CAPS == [15, 16, 17, 32, 33]


def test_ties_at_slip_0():
    lists, _ = pitch(0.0)
    pol = edge_policies()
    for gamma in TIE_GAMMAS:
        for player in (0, 1):
            br, V, Qr, it = brn.best_response(lists, pol, player, gamma, THETA)
            ties = tied_states(Qr, player)
            print("slip 0, discount %.1f, response to player %s: tied states %s" % (gamma, "AB"[player], ties.tolist()))
            assert ties.tolist() == TIE_COUNTS[(gamma, player)]
            # br is the first index that attains the optimum
            best = Qr.min(-1) if player == 0 else Qr.max(-1)
            np.testing.assert_array_equal(br, (Qr == best[..., None]).argmax(-1))


def test_the_rows_are_accepted_or_refused_by_the_documented_rule():
    pol = odd_rows()
    assert all(row_accepted(pol[i, s]) for i in range(2) for s in range(1, NS))
    live = pol[:, 1:]
    assert np.signbit(live[live == 0.0]).sum() > 500            # zeros written as -0.0
    assert ((live > 0.0) & (live < 2.3e-308)).sum() > 500       # subnormal entries
    sums = live.sum(-1)
    assert (sums > 1.0 + 8e-6).sum() > 100 and (sums < 1.0 - 8e-6).sum() > 100 and np.abs(sums - 1.0).max() < 1e-5
    for row, why in refused_rows():
        assert not row_accepted(row) and (row >= 0.0).all(), why
    assert not row_accepted(np.array([0.2, 0.2, np.nan, 0.2, 0.2])) and not row_accepted(np.array([0.3, 0.3, 0.5, -0.1, 0.0]))
    # the restatement solves them in every mode
    lists, starts = pitch(0.2)
    for player in (0, 1):
        assert (brn.best_response(lists, pol, player, 0.9, THETA)[3] < 220).all()
    assert (cpn.cross_play(lists, starts, pol, pol, 0.9, THETA)[1] < 220).all()


@pytest.mark.parametrize("slip", SLIPS)
def test_the_low_discount_matrix_stops_within_its_bound(slip):
    assert PASS_PAIRS == 88128 < PASS_NA * PASS_NB == 89088 and (PASS_NA * PASS_NB - PASS_PAIRS) % 64 == 0
    assert PASS_GAMMA ** (PASS_SWEEPS - 1) < THETA <= PASS_GAMMA ** (PASS_SWEEPS - 2)
    A, B = pass_policies()
    flat = pass_sample()
    assert len(flat) >= 32 and {PASS_PAIRS - 1, PASS_PAIRS, PASS_NA * PASS_NB - 1} <= set(flat)
    payoff, it, V = restated_pairs(slip, A, B, flat, PASS_GAMMA, THETA)
    print("slip %.1f: sweeps of the %d sampled pairs %d .. %d" % (slip, len(flat), it.min(), it.max()))
    assert 2 < it.min() and it.max() <= PASS_SWEEPS
    assert np.abs(payoff).max() > 1e-3
    # the samples of the limit runs
    assert len(boundary_sample(1024)) == 32 and len(boundary_sample(2048)) == 64
    assert {0, 63, 64, 959, 960, 1023} <= set(boundary_sample(1024))
