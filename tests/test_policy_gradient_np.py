"""Where there is no GPU: the numpy restatement of soccer_policy_gradient's definition (tests/policy_gradient_np.py), which
tests/test_gpu_policy_gradient.py pins the device to bit for bit, computes a policy gradient on the oracle's 5x4 lists — the
performance-difference identity holds for both players within the stopping errors of its three solves; a one-hot weight picks
a pair's D * Q; a zero weight changes no bit; a state that is never reached has a normalised gradient of 0.0; the projection
lands on the simplex; a pair of a batch has the bits it has alone."""
import os
import sys

import numpy as np
import pytest

from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_response_np as brn  # noqa: E402
import cross_play_np as cpn  # noqa: E402
import occupancy_np as ocn  # noqa: E402
import policy_gradient_np as pgn  # noqa: E402
from minimax_q_np import shapley_lists  # noqa: E402

GAMMA, THETA = 0.9, 1e-13
SLIPS = [0.0, 0.2]

_games = {}


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def game(slip):
    """(lists, initial states, in-lists, pi_a[2], pi_b[3], the 2 x 3 result with uniform weights) on 5x4, once per slip"""
    if slip not in _games:
        o = Oracle(5, 4, slip, n=1, seed=0)
        lists = shapley_lists(o)
        starts = cpn.isd_obs(o)
        inl = ocn.in_lists_of(lists)
        nS = lists[0].shape[0]
        rng = np.random.default_rng(43)
        A = np.stack([np.full((nS, 5), 0.2), rng.dirichlet(np.ones(5), nS)])
        B = np.stack([np.full((nS, 5), 0.2), rng.dirichlet(np.full(5, 0.5), nS), brn.onehot(rng.integers(0, 5, nS))])
        _games[slip] = (lists, starts, inl, A, B, pgn.policy_gradient(lists, starts, A, B, GAMMA, THETA, inl=inl))
    return _games[slip]


def stopping_bound(nS, gamma, theta):
    """|lhs - rhs| of the identity with three stopped solves: each payoff is off by at most gamma * theta / (1 - gamma) (a
    contraction of modulus gamma stopped at theta), 2 of them; the occupancy lacks at most (nS - 1) * theta * gamma / (1 - gamma)
    in L1 (test_occupancy_np.l1_bound) against an advantage of at most 2 in size; and Q_a, one backup of a V that is off by
    gamma * theta / (1 - gamma), is off by gamma times that, against |D|_1 <= 1 / (1 - gamma) and |x' - x|_1 <= 2"""
    return 2 * gamma * theta / (1 - gamma) + 2 * (nS - 1) * theta * gamma / (1 - gamma) + 2 * gamma ** 2 * theta / (1 - gamma) ** 2


@pytest.mark.parametrize("slip", SLIPS)
def test_the_performance_difference_identity_holds_for_both_players(slip):
    lists, starts, inl, A, B, r = game(slip)
    nS = A.shape[1]
    bound = stopping_bound(nS, GAMMA, THETA)
    assert abs(bound - 1.386e-9) < 1e-12
    x, x2, y, y2 = A[0], A[1], B[1], B[2]
    # player A: payoff(x', y) - payoff(x, y) = sum_s D_{x', y}[s] * sum_a (x'[s][a] - x[s][a]) * Q_a^{x, y}[s][a]
    lhs = r["payoff"][1, 1] - r["payoff"][0, 1]
    adv = ((x2 - x)[1:] * r["q_a"][0, 1, 1:]).sum(1)
    rhs = (r["occupancy"][1, 1, 1:] * adv).sum()
    print("slip %.1f, A: lhs %.12f rhs %.12f diff %.3g (bound %.3g)" % (slip, lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs) > 1e-3 and abs(lhs - rhs) <= bound
    # player B: payoff(x, y') - payoff(x, y) = sum_s D_{x, y'}[s] * sum_b (y'[s][b] - y[s][b]) * Q_b^{x, y}[s][b]
    lhs = r["payoff"][0, 2] - r["payoff"][0, 1]
    adv = ((y2 - y)[1:] * r["q_b"][0, 1, 1:]).sum(1)
    rhs = (r["occupancy"][0, 2, 1:] * adv).sum()
    print("slip %.1f, B: lhs %.12f rhs %.12f diff %.3g (bound %.3g)" % (slip, lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs) > 1e-3 and abs(lhs - rhs) <= bound
    # and the gradient is the identity's first-order term: a small step along a feasible direction moves the payoff by grad . step
    h = 1e-6
    xs = (1 - h) * x + h * x2
    moved = pgn.pairs(lists, starts, xs[None], y[None], GAMMA, THETA, inl=inl)["payoff"][0]
    first_order = h * (r["occupancy"][0, 1, 1:, None] * r["q_a"][0, 1, 1:] * (x2 - x)[1:]).sum()
    print("slip %.1f: payoff moved by %.6g, grad . step %.6g" % (slip, moved - r["payoff"][0, 1], first_order))
    assert abs((moved - r["payoff"][0, 1]) - first_order) <= 2 * bound + 50 * h * h


@pytest.mark.parametrize("slip", SLIPS)
def test_the_weighted_sums(slip):
    lists, starts, inl, A, B, r = game(slip)
    D, qa, qb = r["occupancy"], r["q_a"], r["q_b"]
    assert (qa[:, :, 0] == 0).all() and (qb[:, :, 0] == 0).all() and (D[:, :, 0] == 0).all()
    # a one-hot weight is that pair's D * Q (from 0.0: a -0.0 product becomes +0.0)
    ga, gb, ra, rb = pgn.reduce(D, qa, qb, w_a=[0.0, 1.0], w_b=[0.0, 0.0, 1.0])
    assert (bits(ga) == bits(0.0 + D[:, 2, :, None] * qa[:, 2])).all() and (bits(ra) == bits(0.0 + D[:, 2])).all()
    assert (bits(gb) == bits(0.0 + D[1, :, :, None] * qb[1])).all() and (bits(rb) == bits(0.0 + D[1])).all()
    # a zero weight changes no bit of the other terms' sum
    w = np.array([0.3, 0.0, 0.7])
    with_zero = pgn.reduce(D, qa, qb, w_b=w)
    without = pgn.reduce(D[:, [0, 2]], qa[:, [0, 2]], qb[:, [0, 2]], w_b=w[[0, 2]])
    assert (bits(with_zero[0]) == bits(without[0])).all() and (bits(with_zero[2]) == bits(without[2])).all()
    # uniform weights by default, and the sums are sequential
    ga, gb, ra, rb = pgn.reduce(D, qa, qb)
    third = 1.0 / 3.0
    assert (bits(ra) == bits(((0.0 + third * D[:, 0]) + third * D[:, 1]) + third * D[:, 2])).all()
    assert (bits(gb) == bits((0.0 + 0.5 * (D[0, :, :, None] * qb[0])) + 0.5 * (D[1, :, :, None] * qb[1]))).all()
    assert (bits(ga) == bits(r["grad_a"])).all() and (bits(gb) == bits(r["grad_b"])).all()
    # normalised: grad / reach where the reach is positive
    na = pgn.reduce(D, qa, qb, normalize=True)[0]
    live = ra > 0
    assert live[:, 1:].any() and (bits(na[live]) == bits(ga[live] / ra[live][:, None])).all() and (na[~live] == 0).all()


def test_a_state_that_is_never_reached_has_a_normalised_gradient_of_zero():
    lists, starts, inl, A, B, _ = game(0.0)
    nS = A.shape[1]
    stay = brn.onehot(np.zeros(nS, np.int64))[None]                     # nobody moves: the game never leaves kick-off
    r = pgn.policy_gradient(lists, starts, stay, stay, GAMMA, 1e-10, normalize=True, inl=inl)
    away = np.setdiff1d(np.arange(nS), starts)
    assert (r["occupancy"][0, 0, away] == 0).all() and (r["reach_a"][0, away] == 0).all()
    for g in (r["grad_a"], r["grad_b"]):
        assert (bits(g[0, away]) == 0).all()                            # +0.0, not NaN from 0 / 0
        assert np.isfinite(g).all()
    raw = pgn.policy_gradient(lists, starts, stay, stay, GAMMA, 1e-10, inl=inl)
    assert (bits(r["grad_a"][0, starts]) == bits(raw["grad_a"][0, starts] / raw["reach_a"][0, starts][:, None])).all()


def test_the_projection_lands_on_the_simplex():
    """Two bounds for two kinds of rows.  The rows gradient play projects (a row of the simplex moved by a step of at most 1 in
    every entry, ties, rows of the simplex themselves) sum to 1 within 4 ulp OF 1.0: that is the bound the definition is held
    to.  Rows far outside (entries of size 30) are an addition: every entry of their projection is v - tau rounded at the size
    of v, so they are held to 4 ulp of the row's largest entry, which is no looser for what the first bound covers."""
    rng = np.random.default_rng(5)
    # what gradient play projects: a row of the simplex moved by a step of at most 1 in every entry, so |v| <= 2; rounded ones
    # for ties; and rows of the simplex themselves
    near = np.concatenate([rng.dirichlet(np.ones(5), 4000) + rng.uniform(-1, 1, (4000, 5)), rng.dirichlet(np.ones(5), 1000),
                           np.round(rng.dirichlet(np.ones(5), 1000) + rng.uniform(-1, 1, (1000, 5)), 1)])
    far = rng.normal(0, 30, (1000, 5))
    v = np.concatenate([near, far])
    p = pgn.project(v)
    assert (p >= 0).all() and not np.signbit(p).any()
    eps = np.finfo(np.float64).eps
    err = np.abs(ocn.sequential_sum(p) - 1.0)
    print("max |sum - 1|: %.3g near the simplex, %.3g far from it (%.3g of the row's size)"
          % (err[:6000].max(), err[6000:].max(), (err[6000:] / np.abs(far).max(1)).max()))
    assert err[:6000].max() <= 4 * eps
    # far from the simplex every entry of the result is rounded at the size of v, not of 1
    assert (err[6000:] <= 4 * eps * np.abs(far).max(1)).all()
    # the order of a row's entries does not matter
    perm = rng.permutation(5)
    assert (bits(pgn.project(v[:, perm])) == bits(p[:, perm])).all()
    # the closest point: no other point of the simplex is closer to v than p
    other = rng.dirichlet(np.ones(5), v.shape[0])
    assert (((p - v) ** 2).sum(1) <= ((other - v) ** 2).sum(1) + 1e-9).all()
    # a row on the simplex whose descending sum is exactly 1.0 is returned unchanged, and so is a policy whose direction is 0
    exact = np.array([[0.2] * 5, [1.0, 0, 0, 0, 0], [0, 0, 0.5, 0.25, 0.25], [0, 0.75, 0, 0.25, 0]])
    assert (bits(pgn.project(exact)) == bits(exact)).all()
    x = np.stack([exact] * 2); zero = np.zeros(x.shape)
    x2, y2, pa, pb = pgn.step(x, x, zero, zero, zero, zero, True, 1.0, 8.0, 0.5)
    assert (bits(x2) == bits(x)).all() and (bits(y2) == bits(x)).all()
    # row 0 is never touched
    g = rng.normal(0, 1, x.shape)
    x2, y2, pa, pb = pgn.step(x, x, g, g, zero, zero, True, 1.0, 1.0, 1.0)
    assert (bits(x2[:, 0]) == bits(x[:, 0])).all() and (bits(x2[:, 1:]) != bits(x[:, 1:])).any() and pa is g
    # a side whose step is 0.0 is held fixed to the bit (re-projected, rows whose sum is not exactly 1.0 would drift), its prev follows g
    league = rng.dirichlet(np.ones(5), (2, 50))
    assert (bits(pgn.project(league)) != bits(league)).any()
    x2, y2, pa, pb = pgn.step(x, league, g, rng.normal(0, 1, league.shape), zero, np.zeros(league.shape), False, 1.0, 0.0, 1.0)
    assert (bits(y2) == bits(league)).all() and (bits(x2[:, 1:]) != bits(x[:, 1:])).any() and (pb != 0).all()


def test_a_pair_of_a_batch_has_the_bits_it_has_alone():
    lists, starts, inl, A, B, r = game(0.2)
    alone = pgn.policy_gradient(lists, starts, A[1], B[2], GAMMA, THETA, inl=inl)
    for k in ("payoff", "V", "occupancy", "q_a", "q_b", "iterations"):
        assert (np.asarray(alone[k][0, 0]) == np.asarray(r[k][1, 2])).all(), k
        if r[k].dtype == np.float64:
            assert (bits(alone[k][0, 0]) == bits(r[k][1, 2])).all(), k
    # ... and a policy's gradient against one opponent is its row of a larger call with a one-hot weight
    ga = pgn.reduce(r["occupancy"], r["q_a"], r["q_b"], w_b=[0.0, 0.0, 1.0])[0]
    assert (bits(alone["grad_a"][0]) == bits(ga[1])).all()
    assert r["iterations"].shape == (2, 3, 2) and (r["iterations"] > 100).all()
