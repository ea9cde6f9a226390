"""Minimax (Shapley) value iteration of the two-player game (include/soccer_hip.h, soccer_minimax_value_iteration and
soccer_minimax_backup) restated in numpy over the two-player lists of minimax_q_np.shapley_lists (the CPU oracle's transition
relation): Q is best_response_np.list_q — the definition's float64 arithmetic, sequential from 0.0 in list order — and the
stage games go to the host build of csrc/soccer_games.hpp (test_matrix_game_host.solve_host), which the device build matches
bit for bit.  Row 0 follows the device's definition: its lists are empty, so Q[0] = 0, V[0] = 0 and its strategies are the
zero game's.  tests/test_gpu_two_player_shapes.py and tests/test_gpu_two_player_edges.py hold the device to it bit for bit;
tests/test_minimax_vi_np.py checks what it computes where there is no GPU."""
import numpy as np

from best_response_np import list_q
from test_matrix_game_host import solve_host


def backup(L, lists, V, gamma):
    """one application of Shapley's operator: (pi_a[nS, 5], pi_b[nS, 5], V' = val(Q), Q = Q(V)[nS, 5, 5])"""
    Q = list_q(lists, np.asarray(V, np.float64), gamma)
    Q[0] = 0.0
    v, x, y, _ = solve_host(L, Q)
    v[0] = 0.0
    return x, y, v, Q


def minimax_vi(L, lists, gamma, theta, max_sweeps=1000000):
    """from V_0 = 0: Q_k = Q(V_{k-1}), V_k = val(Q_k) with the strategies of Q_k, until the first k with
    max|V_k - V_{k-1}| < theta or k == max_sweeps.  Returns (pi_a, pi_b, V_k, Q_k, k, capped)."""
    V = np.zeros(lists[0].shape[0])
    for k in range(1, int(max_sweeps) + 1):
        x, y, v, Q = backup(L, lists, V, gamma)
        d = np.abs(v - V).max()
        V = v
        if d < theta:
            return x, y, V, Q, k, False
    return x, y, V, Q, int(max_sweeps), True
