"""Where there is no GPU: the numpy restatement of minimax value iteration (tests/minimax_vi_np.py), which
tests/test_gpu_two_player_shapes.py and tests/test_gpu_two_player_edges.py pin the device to bit for bit, computes what the
definition says — the same fixed point as minimax_q_np.shapley_vi (which sums the lists in another order), a certificate for
every stage game, Q_k = Q(V_{k-1}) with V_k = val(Q_k), and the iterate V_{k-1} at a cap of k - 1."""
import os
import sys

import numpy as np
import pytest

from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import minimax_vi_np as mvn  # noqa: E402
from best_response_np import list_q  # noqa: E402
from minimax_q_np import shapley_lists, shapley_vi  # noqa: E402
from test_matrix_game_host import assert_certificate, build_games_host, solve_host  # noqa: E402

GAMMA, THETA = 0.9, 1e-10
# |V_k - V_{k-1}| <= gamma^(k-1) because |V_1| <= 1: the first k with gamma^(k-1) < theta is 220
SWEEP_BOUND = 220


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_games_host(tmp_path_factory.mktemp("games_vi"))


@pytest.fixture(scope="module", params=[0.0, 0.2])
def solved(request, host):
    """5x4: the lists and the restatement's solve"""
    lists = shapley_lists(Oracle(5, 4, request.param, n=1, seed=0))
    return lists, mvn.minimax_vi(host, lists, GAMMA, THETA)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def test_it_agrees_with_the_shapley_iteration(host, solved):
    lists, (pa, pb, V, Q, k, capped) = solved
    vstar, qstar = shapley_vi(host, lists, GAMMA, THETA)
    gap = np.abs(V - vstar).max()
    print("sweeps %d, max |V - shapley_vi's| %.3g" % (k, gap))
    assert not capped and 16 < k <= SWEEP_BOUND
    assert gap <= 2 * GAMMA * THETA / (1 - GAMMA) + 1e-12      # both are theta-stopped iterates of one contraction
    assert np.abs(V).max() > 0.5 and V[0] == 0.0


def test_every_stage_game_has_its_certificate_and_row_0_is_the_zero_game(host, solved):
    lists, (pa, pb, V, Q, k, capped) = solved
    assert_certificate(Q, V, pa, pb)
    assert (Q[0] == 0.0).all() and V[0] == 0.0
    _, x0, y0, _ = solve_host(host, np.zeros((1, 5, 5)))
    np.testing.assert_array_equal(pa[0], x0[0]); np.testing.assert_array_equal(pb[0], y0[0])
    # the triple is self-consistent: V_k = val(Q_k) with the strategies of Q_k
    v, x, y, _ = solve_host(host, Q)
    np.testing.assert_array_equal(bits(V[1:]), bits(v[1:]))
    np.testing.assert_array_equal(bits(pa), bits(x)); np.testing.assert_array_equal(bits(pb), bits(y))


def test_a_cap_one_below_k_returns_the_iterate_before(host, solved):
    lists, (pa, pb, V, Q, k, capped) = solved
    qa, qb, Vm, Qm, km, capped_m = mvn.minimax_vi(host, lists, GAMMA, THETA, max_sweeps=k - 1)
    assert capped_m and km == k - 1
    assert 0.0 < np.abs(V - Vm).max() < THETA                   # sweep k stopped, and it still moved
    np.testing.assert_array_equal(bits(Q), bits(list_q(lists, Vm, GAMMA)))          # Q_k = Q(V_{k-1})
    ra, rb, Vn, Qn = mvn.backup(host, lists, Vm, GAMMA)                             # and one backup of V_{k-1} is sweep k
    for got, want in ((Vn, V), (Qn, Q), (ra, pa), (rb, pb)):
        np.testing.assert_array_equal(bits(got), bits(want))
    # a cap of k stops where the uncapped solve stops, and is not capped
    again = mvn.minimax_vi(host, lists, GAMMA, THETA, max_sweeps=k)
    assert again[4] == k and not again[5]
    np.testing.assert_array_equal(bits(again[2]), bits(V))
    # by hand, sweep by sweep
    W = np.zeros(V.shape)
    for _ in range(k - 1):
        W, before = mvn.backup(host, lists, W, GAMMA)[2], W
    np.testing.assert_array_equal(bits(W), bits(Vm))
    assert np.abs(W - before).max() >= THETA                    # sweep k - 1 had not stopped
