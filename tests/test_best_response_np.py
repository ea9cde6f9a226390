"""Where there is no GPU: the best-response entry points are part of the C ABI and check their handle first, and the numpy
restatement of their definition (tests/best_response_np.py), which tests/test_gpu_best_response.py pins the device to bit
for bit, computes what a best response must — the equilibrium strategies of a CPU Shapley iteration cannot be exploited,
the uniform policy can, and the sweep count obeys the contraction bound."""
import os
import re
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import _lib
from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_response_np as brn  # noqa: E402
from minimax_q_np import shapley_lists, shapley_vi  # noqa: E402
from test_matrix_game_host import build_games_host, solve_host  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA, THETA = 0.9, 1e-10
# |V_k - V_{k-1}| <= gamma^(k-1) because |V_1| <= 1: the first k with gamma^(k-1) < theta is 220
SWEEP_BOUND = 220


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_games_host(tmp_path_factory.mktemp("games_br"))


@pytest.fixture(scope="module")
def game(host):
    """5x4 at slip 0.2: the lists, V* and the equilibrium strategies of the CPU Shapley iteration"""
    o = Oracle(5, 4, 0.2, n=1, seed=0)
    lists = shapley_lists(o)
    vstar, Q = shapley_vi(host, lists, GAMMA, THETA)
    _, pa, pb, _ = solve_host(host, Q)
    return lists, vstar, pa, pb


def test_symbols_are_declared_exported_and_mirrored():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "soccer_hip.h")).read()
    for name in ("soccer_best_response", "soccer_evaluate_policies"):
        assert re.search(r"\bint %s\(" % name, text), "%s is not declared" % name
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert int(re.search(r"#define\s+SOCCER_BR_MAX_POLICIES\s+(\d+)", text).group(1)) == _lib.BR_MAX_POLICIES == 256
    assert len(_lib.PROTOTYPES["soccer_best_response"][1]) == 11 and len(_lib.PROTOTYPES["soccer_evaluate_policies"][1]) == 9
    assert lib.soccer_abi_version() == 3          # nothing that existed changed


def test_calls_reject_a_null_handle():
    lib = _lib.load()
    pol = np.full((1, 761, 5), 0.2)
    assert lib.soccer_best_response(None, 0, 1, pol.ctypes.data, THETA, GAMMA, 10, None, None, None, None) == _lib.E_INVALID
    assert b"handle is NULL" in lib.soccer_last_error(None)
    assert lib.soccer_evaluate_policies(None, 1, pol.ctypes.data, pol.ctypes.data, THETA, GAMMA, 10, None, None) == _lib.E_INVALID
    assert b"handle is NULL" in lib.soccer_last_error(None)


def test_the_equilibrium_strategies_cannot_be_exploited(game):
    lists, vstar, pa, pb = game
    r = brn.exploitability(lists, pa, pb, GAMMA, THETA)
    v_a, v_b = r["v_a"][0], r["v_b"][0]
    print("max (V* - v_a) %.3g   max (v_b - V*) %.3g   sweeps %s" % ((vstar - v_a)[1:].max(), (v_b - vstar)[1:].max(),
                                                                   [k.tolist() for k in r["iterations"]]))
    assert (v_a[1:] >= vstar[1:] - 1e-6).all() and (v_b[1:] <= vstar[1:] + 1e-6).all()
    assert (r["gap"][0, 1:] <= 2e-6).all()
    assert all((k <= SWEEP_BOUND).all() for k in r["iterations"])
    # the triple is self-consistent, and V[0] is the terminal observation's 0
    br_b, v, Qr, _ = brn.best_response(lists, pa, 0, GAMMA, THETA)
    np.testing.assert_array_equal(v, Qr.min(-1))
    np.testing.assert_array_equal(br_b, Qr.argmin(-1))
    assert v[0, 0] == 0.0 and (Qr[0, 0] == 0.0).all()


def test_the_uniform_policy_can_be_exploited_and_a_batch_changes_nothing(game):
    lists, vstar, pa, pb = game
    uni = np.full(pa.shape, 0.2)
    r = brn.exploitability(lists, uni, uni, GAMMA, THETA)
    gap = r["gap"][0, 1:]
    print("uniform policy: max gap %.4f, sweeps %s" % (gap.max(), [k.tolist() for k in r["iterations"]]))
    assert gap.max() > 1.0 and (gap >= -2 * THETA / (1 - GAMMA)).all()
    assert (r["v_a"][0, 1:] <= vstar[1:] + 1e-6).all() and (r["v_b"][0, 1:] >= vstar[1:] - 1e-6).all()
    assert all((k <= SWEEP_BOUND).all() for k in r["iterations"])
    # solved next to a policy that needs more sweeps, every policy keeps its own bits and its own sweep count
    both = brn.best_response(lists, np.stack([uni, pa]), 0, GAMMA, THETA)
    alone = [brn.best_response(lists, p, 0, GAMMA, THETA) for p in (uni, pa)]
    assert both[3][0] < both[3][1]
    for i in range(2):
        for x, y in zip(both, alone[i]):
            np.testing.assert_array_equal(np.ascontiguousarray(x[i]).view(np.int64), np.ascontiguousarray(y[0]).view(np.int64))
    # too few sweeps for the slower one: it reports max_sweeps, the other one is complete
    m = int(both[3][0]) + 3
    short = brn.best_response(lists, np.stack([uni, pa]), 0, GAMMA, THETA, max_sweeps=m)
    assert short[3].tolist() == [int(both[3][0]), m]
    np.testing.assert_array_equal(short[1][0].view(np.int64), both[1][0].view(np.int64))


def test_a_pair_s_value_lies_between_the_two_responses(game):
    lists, vstar, pa, pb = game
    rng = np.random.default_rng(7)
    x = rng.dirichlet(np.ones(5), pa.shape[0]); y = rng.dirichlet(np.ones(5), pa.shape[0])
    r = brn.exploitability(lists, x, y, GAMMA, THETA)
    V, k = brn.evaluate(lists, x, y, GAMMA, THETA)
    slack = 2 * THETA / (1 - GAMMA)
    assert (V[0] >= r["v_a"][0] - slack).all() and (V[0] <= r["v_b"][0] + slack).all() and k[0] <= SWEEP_BOUND
    # x against B's pure best response to it IS the response value (both theta-converged iterates of one contraction)
    Vb, _ = brn.evaluate(lists, x, brn.onehot(r["br_b"][0]), GAMMA, THETA)
    assert np.abs(Vb[0] - r["v_a"][0]).max() <= 2 * GAMMA * THETA / (1 - GAMMA) + 1e-12
