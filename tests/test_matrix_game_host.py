"""The 5x5 zero-sum matrix-game solver of minimax value iteration (csrc/soccer_games.hpp) on the CPU: the header compiles
for the host (tests/host/games_host.cpp), so this is the code the sweep kernel runs.  Every result must carry its own
certificate (eps = 1e-10 * max(1, max|A|)):  min_b (x^T A)_b >= v - eps,  max_a (A y)_a <= v + eps,  x, y >= 0,
sum x = sum y = 1 within 1e-12; pure saddle points come back exact with the first-index tie rule; closed-form games and
an LP library (where one is installed) pin the value."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_games_host(out_dir):
    so = os.path.join(str(out_dir), "libgames_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           "-o", so, os.path.join(ROOT, "tests", "host", "games_host.cpp")])
    L = C.CDLL(so)
    L.games_solve_host.restype = None
    L.games_solve_host.argtypes = [C.c_long] + [C.c_void_p] * 5
    return L


def solve_host(L, A):
    A = np.ascontiguousarray(A, np.float64).reshape(-1, 5, 5)
    n = A.shape[0]
    v = np.zeros(n); x = np.zeros((n, 5)); y = np.zeros((n, 5)); sad = np.zeros(n, np.int32)
    L.games_solve_host(n, A.ctypes.data, v.ctypes.data, x.ctypes.data, y.ctypes.data, sad.ctypes.data)
    return v, x, y, sad


def hard_games(rng, n_each):
    """games that end the simplex on a basis optimal only to its pivot tolerance: near-ties (small integer games perturbed
    by 1e-15 .. 1e-11), entries of mixed magnitude 1e-8 .. 1e8, rank 1 plus 1e-13 noise"""
    base = rng.integers(-1, 2, (n_each, 5, 5)).astype(np.float64)
    g = [base + rng.choice([1e-15, 1e-13, 1e-11], (n_each, 1, 1)) * rng.integers(-1, 2, (n_each, 5, 5)),
         base + 10.0 ** rng.uniform(-15, -11, (n_each, 1, 1)) * rng.uniform(-1, 1, (n_each, 5, 5)),
         rng.integers(-3, 4, (n_each, 5, 5)) + 1e-12 * rng.integers(-1, 2, (n_each, 5, 5)),
         rng.uniform(-1, 1, (n_each, 5, 5)) * 10.0 ** rng.uniform(-8, 8, (n_each, 5, 5)),
         rng.uniform(-1, 1, (n_each, 5, 1)) * rng.uniform(-1, 1, (n_each, 1, 5)) + 1e-13 * rng.uniform(-1, 1, (n_each, 5, 5))]
    return np.concatenate(g).astype(np.float64)


def game_set(rng, n_each=12500):
    """~1.6e5 games: uniform random, {-1, 0, 1} entries, duplicate / dominated rows and columns, all-zero and constant,
    rank 1, uniform games scaled by 1e-6 and 1e6, and the hard families of hard_games."""
    g = []
    g.append(rng.uniform(-1, 1, (n_each, 5, 5)))
    g.append(rng.integers(-1, 2, (n_each, 5, 5)).astype(np.float64))
    d = rng.uniform(-1, 1, (n_each, 5, 5))
    d[:, 3] = d[:, 1]; d[:, :, 4] = d[:, :, 0]                                   # duplicate row and column
    d[: n_each // 2, 2] = d[: n_each // 2, 0] - rng.uniform(0, 0.5, (n_each // 2, 5))   # dominated row
    d[n_each // 2:, :, 1] = d[n_each // 2:, :, 3] + rng.uniform(0, 0.5, (n_each - n_each // 2, 5))   # dominated column
    g.append(d)
    z = np.zeros((64, 5, 5)); c = np.ones((64, 5, 5)) * rng.uniform(-3, 3, (64, 1, 1))
    g += [z, c]
    u = rng.uniform(-1, 1, (n_each, 5, 1)); w = rng.uniform(-1, 1, (n_each, 1, 5))
    g.append(u * w)                                                                   # rank 1
    g.append(rng.integers(-1, 2, (n_each, 5, 1)) * rng.integers(-1, 2, (n_each, 1, 5)).astype(np.float64))
    g.append(rng.uniform(-1, 1, (n_each, 5, 5)) * 1e-6)
    g.append(rng.uniform(-1, 1, (n_each, 5, 5)) * 1e6)
    # the stage games of the soccer pitch look like this: a few values in [-1, 1], many exact repeats
    g.append(rng.choice(np.array([-1.0, -0.5, 0.0, 0.25, 0.5, 1.0]), (n_each, 5, 5)))
    g.append(hard_games(rng, n_each))
    return np.concatenate(g).astype(np.float64)


def assert_certificate(A, v, x, y):
    A = A.reshape(-1, 5, 5)
    eps = 1e-10 * np.maximum(1.0, np.abs(A).max(axis=(1, 2)))
    assert (x >= 0).all() and (y >= 0).all()
    assert np.abs(x.sum(1) - 1).max() <= 1e-12 and np.abs(y.sum(1) - 1).max() <= 1e-12
    lo = np.einsum("na,nab->nb", x, A).min(1)
    hi = np.einsum("nab,nb->na", A, y).max(1)
    bad = np.flatnonzero((lo < v - eps) | (hi > v + eps))
    assert bad.size == 0, "certificate fails for %d games, first %s: v %r lo %r hi %r" % (
        bad.size, A[bad[0]].tolist(), v[bad[0]], lo[bad[0]], hi[bad[0]])


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_games_host(tmp_path_factory.mktemp("games"))


def test_accuracy_contract_on_1e5_games(host):
    A = game_set(np.random.default_rng(1994))
    assert A.shape[0] >= 100000
    v, x, y, sad = solve_host(host, A)
    assert_certificate(A, v, x, y)
    assert set(np.unique(sad).tolist()) == {0, 1, 2}    # simplex, saddle point and the enumeration fallback all occur


def test_hard_families_need_the_fallback_and_meet_the_contract(host):
    """2e5 near-tie, mixed-magnitude and rank-1-plus-noise games: the simplex alone leaves brackets up to ~1e4 eps wide on
    some of them; every returned triple must still pass"""
    A = hard_games(np.random.default_rng(2024), 40000)
    v, x, y, sad = solve_host(host, A)
    assert_certificate(A, v, x, y)
    assert (sad == 2).sum() > 1000 and not (sad == 3).any()


def test_pure_saddle_points_are_exact_with_the_first_index_rule(host):
    A = game_set(np.random.default_rng(7))
    v, x, y, sad = solve_host(host, A)
    rowmin = A.min(2); colmax = A.max(1)
    maxmin = rowmin.max(1); minmax = colmax.min(1)
    pure = maxmin == minmax
    np.testing.assert_array_equal(sad == 1, pure)
    a_star = np.argmax(rowmin == maxmin[:, None], axis=1)            # first row whose minimum is the max-min
    b_star = np.argmax(colmax == minmax[:, None], axis=1)            # first column whose maximum is the min-max
    idx = np.flatnonzero(pure)
    np.testing.assert_array_equal(v[idx].view(np.int64), A[idx, a_star[idx], b_star[idx]].view(np.int64))
    np.testing.assert_array_equal(x[idx], np.eye(5)[a_star[idx]])
    np.testing.assert_array_equal(y[idx], np.eye(5)[b_star[idx]])
    # ties: an all-zero game is e_0 / e_0; a game whose rows 1 and 3 both reach the max-min and whose columns 2, 3 and 4
    # all reach the min-max picks row 1 and column 2
    t = np.full((1, 5, 5), -1.0); t[0, 1] = 0.0; t[0, 3] = 0.0; t[0, :, 0] = 1.0; t[0, :, 1] = 1.0
    v, x, y, sad = solve_host(host, np.concatenate([np.zeros((1, 5, 5)), t]))
    assert sad.tolist() == [1, 1] and v.tolist() == [0.0, 0.0]
    np.testing.assert_array_equal(x, np.eye(5)[[0, 1]]); np.testing.assert_array_equal(y, np.eye(5)[[0, 2]])


def test_closed_forms(host):
    mp = np.full((5, 5), -2.0)                          # matching pennies among dominated actions
    mp[:2, :2] = [[1.0, -1.0], [-1.0, 1.0]]
    mp[:, 2:] = 2.0                                     # B never plays 2..4 (A wins 2 there) ...
    mp[2:, :2] = -2.0                                   # ... and A never plays 2..4
    rps = np.full((5, 5), 2.0)
    rps[:3, :3] = [[0, -1, 1], [1, 0, -1], [-1, 1, 0]]
    rps[3:, :] = -2.0; rps[:3, 3:] = 2.0
    cyc = np.zeros((5, 5))                              # the 5-cycle: i beats i+1 and i+3, loses to i+2 and i+4
    for i in range(5):
        cyc[i, (i + 1) % 5] = cyc[i, (i + 3) % 5] = 1.0
        cyc[i, (i + 2) % 5] = cyc[i, (i + 4) % 5] = -1.0
    v, x, y, sad = solve_host(host, np.stack([mp, rps, cyc]))
    assert sad.tolist() == [0, 0, 0]
    np.testing.assert_allclose(v, [0.0, 0.0, 0.0], atol=1e-14)
    np.testing.assert_allclose(x[0], [0.5, 0.5, 0, 0, 0], atol=1e-14)
    np.testing.assert_allclose(y[0], [0.5, 0.5, 0, 0, 0], atol=1e-14)
    np.testing.assert_allclose(x[1], [1 / 3, 1 / 3, 1 / 3, 0, 0], atol=1e-14)
    np.testing.assert_allclose(y[1], [1 / 3, 1 / 3, 1 / 3, 0, 0], atol=1e-14)
    np.testing.assert_allclose(x[2], [0.2] * 5, atol=1e-14)
    np.testing.assert_allclose(y[2], [0.2] * 5, atol=1e-14)


def test_same_bits_every_time(host):
    A = game_set(np.random.default_rng(3), n_each=2000)
    r1 = solve_host(host, A); r2 = solve_host(host, A[::-1].copy())
    for a, b in zip(r1, r2):
        np.testing.assert_array_equal(a, b[::-1])


def test_value_against_an_lp_library(host):
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(11)
    A = np.concatenate([rng.uniform(-1, 1, (150, 5, 5)), rng.integers(-1, 2, (150, 5, 5)).astype(np.float64)])
    v, _, _, _ = solve_host(host, A)
    for g in range(A.shape[0]):
        # max v  s.t.  x^T A[:, b] >= v for all b,  sum x = 1,  x >= 0   (variables x0..x4, v)
        c = np.zeros(6); c[5] = -1.0
        A_ub = np.hstack([-A[g].T, np.ones((5, 1))]); b_ub = np.zeros(5)
        A_eq = np.array([[1.0] * 5 + [0.0]]); b_eq = np.array([1.0])
        r = opt.linprog(c, A_ub=A_ub, b_ub=b_ub, A_eq=A_eq, b_eq=b_eq, bounds=[(0, None)] * 5 + [(None, None)], method="highs")
        assert r.status == 0
        assert abs(-r.fun - v[g]) <= 1e-9, (g, -r.fun, v[g])
