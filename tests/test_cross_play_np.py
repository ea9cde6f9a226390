"""Where there is no GPU: soccer_cross_play is part of the C ABI and checks its handle first, and the numpy restatement of
its definition (tests/cross_play_np.py), which tests/test_gpu_cross_play.py pins the device to bit for bit, computes what a
payoff matrix must — every entry lies between the worst cases of its two policies, and the equilibrium pair's entry is the
game's value."""
import os
import re
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import _lib
from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_response_np as brn  # noqa: E402
import cross_play_np as cpn  # noqa: E402
from minimax_q_np import shapley_lists, shapley_vi  # noqa: E402
from test_matrix_game_host import build_games_host, solve_host  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA, THETA = 0.9, 1e-10
# two fixed points of contractions with modulus gamma, each stopped at max|V_k - V_{k-1}| < theta
MARGIN = 2 * GAMMA * THETA / (1 - GAMMA)


@pytest.fixture(scope="module")
def game(tmp_path_factory):
    """5x4 at slip 0.2: the lists, the initial states, V* and the equilibrium strategies of the CPU Shapley iteration"""
    host = build_games_host(tmp_path_factory.mktemp("games_cross"))
    o = Oracle(5, 4, 0.2, n=1, seed=0)
    lists = shapley_lists(o)
    vstar, Q = shapley_vi(host, lists, GAMMA, THETA)
    _, pa, pb, _ = solve_host(host, Q)
    return lists, cpn.isd_obs(o), vstar, pa, pb


def test_the_symbol_is_declared_exported_and_mirrored():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "soccer_hip.h")).read()
    assert re.search(r"\bint soccer_cross_play\(", text), "soccer_cross_play is not declared"
    assert "soccer_cross_play" in _lib.PROTOTYPES and hasattr(lib, "soccer_cross_play")
    assert int(re.search(r"#define\s+SOCCER_CROSS_MAX_POLICIES\s+(\d+)", text).group(1)) == _lib.CROSS_MAX_POLICIES == 1024
    assert len(_lib.PROTOTYPES["soccer_cross_play"][1]) == 12
    assert "soccer_cross_play" in re.search(r"#define SOCCER_ABI_VERSION 3.*?\*/", text, re.S).group(0)
    assert lib.soccer_abi_version() == 3          # nothing that existed changed


@pytest.mark.parametrize("n_a,n_b,theta,gamma,sweeps,ppp", [
    (1, 1, THETA, GAMMA, 10, 0), (0, 1, THETA, GAMMA, 10, 0), (1, 1025, THETA, GAMMA, 10, 0), (1, 1, -1.0, GAMMA, 10, 0),
    (1, 1, THETA, 1.5, 10, 0), (1, 1, THETA, GAMMA, 0, 0), (1, 1, THETA, GAMMA, 10, 65)])
def test_the_call_rejects_a_null_handle_whatever_else_it_is_given(n_a, n_b, theta, gamma, sweeps, ppp):
    lib = _lib.load()
    pol = np.full((1, 761, 5), 0.2)
    out = np.full(1, 7.0)
    assert lib.soccer_cross_play(None, n_a, pol.ctypes.data, n_b, pol.ctypes.data, theta, gamma, sweeps, ppp, out.ctypes.data,
                                 None, None) == _lib.E_INVALID
    assert b"handle is NULL" in lib.soccer_last_error(None)
    assert out[0] == 7.0


def test_every_entry_lies_between_its_two_policies_worst_cases(game):
    lists, starts, vstar, pa, pb = game
    nS = pa.shape[0]
    rng = np.random.default_rng(5)
    A = np.stack([np.full((nS, 5), 0.2), pa, rng.dirichlet(np.ones(5), nS), brn.onehot(rng.integers(0, 5, nS))])
    B = np.stack([np.full((nS, 5), 0.2), pb, rng.dirichlet(np.ones(5), nS), brn.onehot(rng.integers(0, 5, nS))])
    payoff, it, V = cpn.cross_play(lists, starts, A, B, GAMMA, THETA)
    assert payoff.shape == it.shape == (4, 4) and V.shape == (4, 4, nS) and (V[:, :, 0] == 0).all()
    # the definition, entry by entry: each pair alone, and the mean over the initial states
    assert len(starts) in (2, 4) and len(set(starts)) == len(starts)
    for i, j in ((0, 0), (1, 2), (3, 1)):
        v, k = brn.evaluate(lists, A[i], B[j], GAMMA, THETA)
        np.testing.assert_array_equal(V[i, j].view(np.int64), v[0].view(np.int64))
        assert it[i, j] == k[0]
        want = 0.0
        for s in starts:
            want = want + v[0, s]
        assert payoff[i, j] == want / len(starts)
    assert it.min() < it.max(), "the pairs should stop at different sweeps"
    lo = cpn.kickoff(brn.best_response(lists, A, 0, GAMMA, THETA)[1], starts)        # each A policy's worst case
    hi = cpn.kickoff(brn.best_response(lists, B, 1, GAMMA, THETA)[1], starts)        # each B policy's
    print("payoff\n%s\nworst cases of A's %s, of B's %s, sweeps %s" % (np.round(payoff, 4), np.round(lo, 4), np.round(hi, 4), it.tolist()))
    assert (payoff >= lo[:, None] - MARGIN).all() and (payoff <= hi[None, :] + MARGIN).all()
    # state by state as well
    v_a = brn.best_response(lists, A, 0, GAMMA, THETA)[1]; v_b = brn.best_response(lists, B, 1, GAMMA, THETA)[1]
    assert (V >= v_a[:, None, :] - MARGIN).all() and (V <= v_b[None, :, :] + MARGIN).all()
    # the equilibrium pair meets at the game's value (shapley_vi's V* is itself stopped at theta)
    vs = cpn.kickoff(vstar, starts)
    print("equilibrium pair %.3e, V* %.3e, margin %.3e" % (payoff[1, 1], vs, MARGIN))
    assert abs(payoff[1, 1] - vs) <= MARGIN
    # the maximin strategy is the row with the best worst opponent in the set, and symmetrically
    assert payoff.min(1).argmax() == 1 and payoff.max(0).argmin() == 1
