"""-m gpu: planners.psro — the loop of cross-play, the meta-game and league challengers.  What it returns is held to what it
says it computes (the matrix is the full cross_play of the returned sets bit for bit, the picks are first argmax / argmin,
additions follow the strict comparisons, mixtures have the length of their set), two runs from one seed agree in every bit,
and from the equilibrium of minimax value iteration no challenger gets past the error of a solve stopped at theta."""
import numpy as np
import pytest

from gym_soccer_littman94_amd import VectorSoccerEnv
from gym_soccer_littman94_amd import planners as pl

pytestmark = pytest.mark.gpu

GAMMA, THETA, SEED = 0.9, 1e-10, 1994
N, ITERATIONS, N_STEPS = 67, 2, 300


def run_psro(**kw):
    env = VectorSoccerEnv(N, 5, 4, 0.2, seed=SEED, autoreset=True)
    out = pl.psro(env, ITERATIONS, N_STEPS, GAMMA, theta=THETA, **kw)
    return env, out


def bits(x):
    return np.ascontiguousarray(x).tobytes()


def test_psro_returns_what_it_says_it_computes_and_is_a_function_of_the_seed():
    env, r = run_psro()
    env2, r2 = run_psro()
    assert set(r) == {"pi_a", "pi_b", "payoff", "iterations", "x", "y", "lo", "hi", "status", "u_a", "u_b", "chosen_a", "chosen_b",
                      "added_a", "added_b", "br_a", "br_b", "gap"}
    for k in r:                                                         # two runs from the same seed: every array, bit for bit
        if isinstance(r[k], list):
            assert len(r[k]) == len(r2[k]) == ITERATIONS and all(bits(a) == bits(b) for a, b in zip(r[k], r2[k])), k
        else:
            assert r[k].shape == r2[k].shape and bits(r[k]) == bits(r2[k]), k
    env2.close()
    nS = env.nS
    # the assembled matrix is the full cross-play of the returned sets
    full = pl.cross_play(env, r["pi_a"], r["pi_b"], THETA, GAMMA)
    assert r["payoff"].shape == (r["pi_a"].shape[0], r["pi_b"].shape[0])
    assert bits(r["payoff"]) == bits(full["payoff"]) and np.array_equal(r["iterations"], full["iterations"])
    assert r["u_a"].shape == r["u_b"].shape == (ITERATIONS, N)
    size_a, size_b = 1, 1                                               # the seeds: one uniform policy a side
    assert bits(r["pi_a"][0]) == bits(np.full((nS, 5), 0.2)) and bits(r["pi_b"][0]) == bits(np.full((nS, 5), 0.2))
    for k in range(ITERATIONS):
        x, y, lo, hi = r["x"][k], r["y"][k], r["lo"][k], r["hi"][k]
        print("iteration %d: |Pi_A| = %d, |Pi_B| = %d, lo %.6f hi %.6f, br_a %.6f br_b %.6f, gap %.6f, added %s / %s"
              % (k, size_a, size_b, lo, hi, r["br_a"][k], r["br_b"][k], r["gap"][k], r["added_a"][k], r["added_b"][k]))
        assert x.shape == (size_a,) and y.shape == (size_b,)
        assert (x >= 0).all() and (y >= 0).all() and abs(x.sum() - 1) <= 1e-12 and abs(y.sum() - 1) <= 1e-12    # the solver's guarantee
        assert lo <= hi and r["status"][k] in (0, 1, 2)
        assert r["chosen_a"][k] == int(np.argmax(r["u_a"][k])) and r["chosen_b"][k] == int(np.argmin(r["u_b"][k]))
        assert r["br_a"][k] == r["u_a"][k].max() and r["br_b"][k] == r["u_b"][k].min()
        assert r["gap"][k] == r["br_a"][k] - r["br_b"][k]
        assert r["added_a"][k] == bool(r["u_a"][k].max() > hi) and r["added_b"][k] == bool(r["u_b"][k].min() < lo)
        size_a += int(r["added_a"][k]); size_b += int(r["added_b"][k])
    assert r["pi_a"].shape == (size_a, nS, 5) and r["pi_b"].shape == (size_b, nS, 5)
    for pi in (r["pi_a"][1:], r["pi_b"][1:]):                           # every added policy is one-hot in every row
        assert np.isin(pi, (0.0, 1.0)).all() and (pi.sum(2) == 1.0).all()
    assert sum(r["added_a"]) + sum(r["added_b"]) > 0                    # against a uniform seed a learner finds something
    env.close()


def test_from_the_minimax_equilibrium_no_challenger_gets_past_the_error_of_the_solve():
    """Seeds: the strategies of minimax value iteration stopped at theta.  The bound, from theta and gamma alone:
    the iteration stops when a sweep moves V by less than theta, so the V its strategies are solved from is within
    eps = theta / (1 - gamma) of the game's value V*.  pi_b solves the stage games of that V exactly, so the value U of
    player A's best response to pi_b obeys |U - V*| <= gamma * |U - V*| + 2 * gamma * eps, i.e. |U - V*| <= 2 * gamma * eps /
    (1 - gamma) in every state, hence at kick-off; likewise for pi_a's worst case.  The pair's own value, which is lo = hi
    of the 1 x 1 meta-game, lies between the two worst cases, and every cross-play entry is a policy evaluation stopped at
    theta, off by at most eps.  So for every challenger of A:  u_a <= U + eps <= V* + 2 gamma eps / (1 - gamma) + eps  and
    hi >= V* - 2 gamma eps / (1 - gamma) - eps,  together  u_a - hi <= margin = 4 gamma theta / (1 - gamma)^2 + 2 theta /
    (1 - gamma)  = 3.8e-8 here; and lo - u_b <= margin for every challenger of B."""
    env = VectorSoccerEnv(N, 5, 4, 0.2, seed=SEED, autoreset=True)
    pi_a, pi_b = pl.minimax_value_iteration(env, THETA, GAMMA)[:2]
    r = pl.psro(env, ITERATIONS, N_STEPS, GAMMA, theta=THETA, pi_a0=pi_a, pi_b0=pi_b)
    margin = 4.0 * GAMMA * THETA / (1.0 - GAMMA) ** 2 + 2.0 * THETA / (1.0 - GAMMA)
    for k in range(ITERATIONS):
        print("iteration %d: lo %.12f hi %.12f, u_a.max() - hi = %.3e, lo - u_b.min() = %.3e (margin %.3e)"
              % (k, r["lo"][k], r["hi"][k], r["u_a"][k].max() - r["hi"][k], r["lo"][k] - r["u_b"][k].min(), margin))
    v_eq = r["payoff"][0, 0]                                            # the equilibrium pair's own value at kick-off
    checked = 0
    for k in range(ITERATIONS):
        # the derivation holds while the league IS the equilibrium strategy: a policy added inside the margin (the strict
        # comparison of step 5 has no margin) makes the later mixtures another opponent
        if any(r["added_a"][:k]) or any(r["added_b"][:k]):
            break
        assert r["x"][k].tolist() == [1.0] and r["y"][k].tolist() == [1.0] and r["lo"][k] == r["hi"][k] == v_eq
        assert r["u_a"][k].max() <= v_eq + margin
        assert r["u_b"][k].min() >= v_eq - margin
        checked += 1
    assert checked >= 1
    env.close()
