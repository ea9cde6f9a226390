"""CPU: the restatement of the league opponent (tests/league_np.py) against what it must reduce to, the pick function at its
boundary words, the compiled host threshold builder and bisection (csrc/soccer_league.hpp through tests/host/league_host.cpp)
against numpy integer for integer, and the frequencies of the kick-off draw."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from league_np import QLeagueNumpy, league_pick, league_thresholds  # noqa: E402
from philox_np import lane_words  # noqa: E402
from q_population_np import QPopulationNumpy, assert_population_equal  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA, SEED, T_RUN = 0.9, 1994, 60
RUN_KW = dict(explor=0.2, decay=0.99)

# the weight vectors of the boundary tests: leading zeros, inner zeros, a trailing zero, a sum of 1 + 9e-6, one policy, two
WEIGHTS = {
    "leading zeros": [0.0, 0.0, 0.25, 0.75],
    "inner zeros": [0.5, 0.0, 0.0, 0.125, 0.0, 0.375],
    "trailing zero": [0.25, 0.75, 0.0],
    "sum 1 + 9e-6": [0.3, 0.3, 0.4 + 9e-6, 0.0],
    "uneven": [0.1, 0.2, 0.3, 0.4],
    "one": [1.0],
    "two": [1.0 / 3.0, 2.0 / 3.0],
}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("league_host")), "libleague_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           "-o", so, os.path.join(ROOT, "tests", "host", "league_host.cpp")])
    L = C.CDLL(so)
    L.league_check_host.restype = C.c_int
    L.league_check_host.argtypes = [C.c_void_p, C.c_int]
    L.league_thresholds_host.restype = None
    L.league_thresholds_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.league_pick_host.restype = None
    L.league_pick_host.argtypes = [C.c_void_p, C.c_int, C.c_long, C.c_void_p, C.c_void_p]
    return L


def boundary_words(T):
    """0, 2^32 - 1 and both sides of every threshold that a 32-bit word can reach"""
    w = {0, 2 ** 32 - 1}
    for t in T.tolist():
        w |= {x for x in (t - 1, t, t + 1) if 0 <= x < 2 ** 32}
    return np.array(sorted(w), np.uint64).astype(np.uint32)


def first_exceeding(weights, W):
    """the pick spelled the other way round: the first k < K - 1 whose threshold exceeds W, K - 1 if none does"""
    T = league_thresholds(weights).tolist()
    return next((k for k, t in enumerate(T) if int(W) < t), len(T))


# ---- 1. what the restatement must reduce to ---------------------------------------------------------------
@pytest.mark.parametrize("player", [0, 1])
@pytest.mark.parametrize("case", ["K=1", "K=3, weights (0, 1, 0)"])
def test_a_league_of_one_live_policy_is_the_fixed_population_bit_for_bit(player, case):
    n = 67
    o1 = Oracle(5, 4, 0.2, n=n, seed=SEED, autoreset=True, max_steps=5)
    o2 = Oracle(5, 4, 0.2, n=n, seed=SEED, autoreset=True, max_steps=5)
    rng = np.random.default_rng(5)
    pols = rng.dirichlet(np.ones(5), (3, o1.nS))
    fixed = pols[1]
    acts = dict(act_a=fixed, act_b="greedy") if player == 0 else dict(act_a="greedy", act_b=fixed)
    want = QPopulationNumpy(n, o1.nS, GAMMA, **acts, **RUN_KW)
    want.run(o1, o1.reset(), T_RUN)
    got = QLeagueNumpy(n, o2.nS, GAMMA, player, pols[1:2] if case == "K=1" else pols, [1.0] if case == "K=1" else [0.0, 1.0, 0.0],
                       other="greedy", **RUN_KW)
    got.run(o2, o2.reset(), T_RUN)
    assert_population_equal(got.state(), want.state())
    assert want.n_truncated_only > 0 and got.n_redraws > 0
    live = got.pick[got.pick >= 0]
    assert (live == (0 if case == "K=1" else 1)).all()


# ---- 2. the pick function at its boundaries ------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(WEIGHTS))
def test_pick_at_the_boundary_words(name):
    w = WEIGHTS[name]
    K = len(w)
    T = league_thresholds(w)
    assert T.size == K - 1 and (np.diff(T.astype(np.int64)) >= 0).all() and (T <= 2 ** 32).all()
    words = boundary_words(T)
    pick = league_pick(T, words)
    np.testing.assert_array_equal(pick, [first_exceeding(w, W) for W in words.tolist()])
    assert pick.min() >= 0 and pick.max() <= K - 1
    zero = [k for k in range(K) if w[k] == 0.0 and k < K - 1]
    assert not np.isin(pick, zero).any()                    # a zero-weight policy before the last is never picked
    for k, t in enumerate(T.tolist()):                      # T_k - 1 still picks at most k, T_k picks more than k
        if 0 < t < 2 ** 32:
            assert league_pick(T, [t - 1])[0] <= k < league_pick(T, [t])[0]


def test_named_boundaries():
    assert league_thresholds(WEIGHTS["leading zeros"]).tolist() == [0, 0, 2 ** 30]
    assert league_pick(league_thresholds(WEIGHTS["leading zeros"]), [0, 2 ** 30 - 1, 2 ** 30, 2 ** 32 - 1]).tolist() == [2, 2, 3, 3]
    T = league_thresholds(WEIGHTS["inner zeros"])
    assert T.tolist() == [2 ** 31, 2 ** 31, 2 ** 31, 5 * 2 ** 29, 5 * 2 ** 29]
    assert league_pick(T, [0, 2 ** 31 - 1, 2 ** 31, 5 * 2 ** 29 - 1, 5 * 2 ** 29, 2 ** 32 - 1]).tolist() == [0, 0, 3, 3, 5, 5]
    # a trailing zero: c_{K-2} = 1.0, T = 2^32, which no 32-bit word reaches — the last policy is unreachable
    T = league_thresholds(WEIGHTS["trailing zero"])
    assert T.tolist() == [2 ** 30, 2 ** 32] and league_pick(T, [2 ** 30 - 1, 2 ** 30, 2 ** 32 - 1]).tolist() == [0, 1, 1]
    # a sum of 1 + 9e-6 (inside the tolerance): the last threshold is clamped to 2^32, not beyond
    T = league_thresholds(WEIGHTS["sum 1 + 9e-6"])
    assert T[-1] == 2 ** 32 and league_pick(T, [2 ** 32 - 1])[0] == 2
    assert league_thresholds([1.0]).size == 0 and league_pick(league_thresholds([1.0]), [0, 2 ** 32 - 1]).tolist() == [0, 0]


# ---- 3. the compiled builder ---------------------------------------------------------------------------------
def test_the_compiled_threshold_builder_and_bisection_agree_with_numpy(host):
    rng = np.random.default_rng(7)
    big = rng.dirichlet(np.ones(1024)); big[rng.random(1024) < 0.3] = 0.0; big /= big.sum()
    cases = dict(WEIGHTS, big=big.tolist(), flat1024=[1.0 / 1024] * 1024)
    for name, w in cases.items():
        w = np.ascontiguousarray(w, np.float64)
        K = w.size
        assert host.league_check_host(w.ctypes.data, K) == -1, name
        T = np.zeros(max(K - 1, 1), np.uint64)
        host.league_thresholds_host(w.ctypes.data, K, T.ctypes.data)
        want = league_thresholds(w)
        np.testing.assert_array_equal(T[:K - 1], want, err_msg=name)
        words = np.concatenate([boundary_words(want), rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)])
        pick = np.zeros(words.size, np.int32)
        host.league_pick_host(T.ctypes.data, K, words.size, words.ctypes.data, pick.ctypes.data)
        np.testing.assert_array_equal(pick, league_pick(want, words), err_msg=name)
    # the checks: the first bad index, K for a bad sum
    for w, code in (([0.5, -0.1, 0.6], 1), ([0.5, float("nan"), 0.5], 1), ([float("inf"), 0.0], 0), ([0.5, 0.5 + 1.2e-5], 2),
                    ([0.5, 0.5 - 1.2e-5], 2), ([0.5, 0.5 + 9e-6], -1)):
        w = np.ascontiguousarray(w, np.float64)
        assert host.league_check_host(w.ctypes.data, w.size) == code, w


# ---- 4. the draw's frequencies -------------------------------------------------------------------------------
def test_frequencies_over_65536_lanes_lie_within_five_binomial_standard_deviations():
    w = np.array([0.1, 0.2, 0.3, 0.4])
    N = 2 ** 16
    T = league_thresholds(w)
    for tick, offset in ((0, 0), (7, 12345)):
        W = lane_words(SEED, offset + np.arange(N), 2 ** 62 + tick, purpose=1)
        counts = np.bincount(league_pick(T, W), minlength=4)
        sd = np.sqrt(N * w * (1.0 - w))
        print("tick %d: counts %s, expected %s, 5 sd %s" % (tick, counts.tolist(), (N * w).tolist(), np.round(5 * sd, 1).tolist()))
        assert counts.sum() == N and (np.abs(counts - N * w) <= 5.0 * sd).all()
