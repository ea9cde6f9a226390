"""Where there is no GPU: the numpy restatement of soccer_match_outcomes' definition (tests/match_outcomes_np.py), which
tests/test_gpu_match_outcomes.py pins the device to bit for bit, computes what win, loss and draw odds and a game length must
on the oracle's 5x4 lists — the win margin is cross-play's value, the three outcomes' probabilities add up to one, a pair that
never moves plays exactly as long as it is allowed to, and a pair of a batch has the bits it has alone."""
import os
import sys

import numpy as np
import pytest

from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_response_np as brn  # noqa: E402
import cross_play_np as cpn  # noqa: E402
import match_outcomes_np as mon  # noqa: E402
from minimax_q_np import shapley_lists  # noqa: E402

THETA, C = 1e-10, 0.9
SLIPS = [0.0, 0.2]
# three fixed points of contractions with modulus c, each stopped at max|F_k - F_{k-1}| < theta
MARGIN = 3 * C * THETA / (1 - C)
# c * (W_A + W_B) + (1 - c) * L = 1 at the fixed points: the same stopping error, weighted
CONSERVED = (2 * C + (1 - C)) * C * THETA / (1 - C)

_games = {}


def game(slip):
    """(lists, initial states, pi_a[3], pi_b[2], the 3 x 2 result) on 5x4, computed once per slip"""
    if slip not in _games:
        o = Oracle(5, 4, slip, n=1, seed=0)
        lists = shapley_lists(o)
        starts = cpn.isd_obs(o)
        nS = lists[0].shape[0]
        rng = np.random.default_rng(41)
        A = np.stack([np.full((nS, 5), 0.2), rng.dirichlet(np.ones(5), nS), brn.onehot(rng.integers(0, 5, nS))])
        B = np.stack([np.full((nS, 5), 0.2), rng.dirichlet(np.full(5, 0.2), nS)])
        _games[slip] = (lists, starts, A, B, mon.match_outcomes(lists, starts, A, B, C, THETA))
    return _games[slip]


def noop(nS):
    return brn.onehot(np.zeros(nS, np.int64))


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


@pytest.mark.parametrize("slip", SLIPS)
def test_the_win_margin_is_the_discounted_value_and_the_outcomes_add_up(slip):
    lists, starts, A, B, r = game(slip)
    F, it = r["values"], r["iterations"]
    nS = F.shape[-1]
    assert F.shape == (3, 2, 3, nS) and it.shape == (3, 2) and (F[:, :, :, 0] == 0).all()
    print("slip %.1f: sweeps %s\nwin_a\n%s\nwin_b\n%s\nlength\n%s" % (slip, it.tolist(), r["win_a"], r["win_b"], r["length"]))
    # no channel moves by more than c^(k-1) in sweep k (L_1 <= 1): below theta from k = 220 on, one more for rounding
    assert it.max() <= 221
    V = cpn.cross_play(lists, starts, A, B, C, THETA)[2]
    err = np.abs((F[:, :, 0] - F[:, :, 1]) - V).max()
    cons = np.abs(C * (F[:, :, 0] + F[:, :, 1]) + (1 - C) * F[:, :, 2] - 1.0)[:, :, 1:].max()
    print("max |(W_A - W_B) - V| %.3g (bound %.3g), conservation %.3g (bound %.3g)" % (err, MARGIN, cons, CONSERVED))
    assert err <= MARGIN and cons <= CONSERVED
    # probabilities, and a game of at least one step and at most 1 / (1 - c)
    assert (F[:, :, :2] >= 0).all() and (F[:, :, 0] + F[:, :, 1] <= 1 + MARGIN).all()
    # (a list's probabilities and a policy's row sum to 1 only up to rounding)
    assert (F[:, :, 2, 1:] >= 1.0 - 1e-12).all() and (F[:, :, 2] <= 1 / (1 - C) + MARGIN).all()
    # the kick-off numbers are the sequential mean over the initial states
    for name, ch in (("win_a", 0), ("win_b", 1), ("length", 2)):
        want = np.zeros((3, 2))
        for s in starts:
            want = want + F[:, :, ch, s]
        np.testing.assert_array_equal(bits(r[name]), bits(want / len(starts)))


@pytest.mark.parametrize("slip", SLIPS)
def test_uniform_against_uniform_is_even(slip):
    _, _, _, _, r = game(slip)
    wa, wb, L = r["win_a"][0, 0], r["win_b"][0, 0], r["length"][0, 0]
    print("slip %.1f, uniform against uniform: win_a %.6f win_b %.6f length %.6f" % (slip, wa, wb, L))
    # the game is symmetric under swapping the sides, so only rounding separates the two: at most some 40 roundings of
    # numbers below 1 per sweep, which the contraction sums to 40 * 2^-53 / (1 - c) < 1e-13
    assert abs(wa - wb) <= 1e-13 and 0.05 < wa < 0.2 and 7.0 < L < 9.0


def test_a_pair_that_never_moves_plays_as_long_as_it_may():
    lists, starts, _, _, _ = game(0.0)
    nS = lists[0].shape[0]
    r = mon.match_outcomes(lists, starts, noop(nS), noop(nS), 1.0, THETA, max_sweeps=37)
    F = r["values"][0, 0]
    assert r["iterations"][0, 0] == 37
    assert (F[:2] == 0).all() and (F[2, 1:] == 37.0).all() and F[2, 0] == 0
    assert r["length"][0, 0] == 37.0 and r["win_a"][0, 0] == 0 and r["win_b"][0, 0] == 0
    r = mon.match_outcomes(lists, starts, noop(nS), noop(nS), C, THETA, max_sweeps=37)
    F = r["values"][0, 0]
    want = (1 - C ** 37) / (1 - C)
    print("NOOP against NOOP at c = 0.9, 37 sweeps: length %.10f, (1 - c^37) / (1 - c) = %.10f" % (r["length"][0, 0], want))
    # 37 steps of L = 1 + c * L below 10, three roundings each
    assert np.abs(F[2, 1:] - want).max() <= 37 * 3 * 10 * 2.0 ** -53 and (F[:2] == 0).all()


def test_each_channel_is_the_pair_evaluation_with_another_reward():
    """W_A, W_B and L are best_response_np's evaluation sweep over lists whose reward is (reward > 0), (reward < 0) and 1.0:
    the same sums in the same order, so the same bits — here for 12 sweeps, which the joint stopping rule does not end"""
    lists, starts, A, B, _ = game(0.2)
    Pp, Pn, Pr, Pd = lists
    x = brn._policies(A[[0, 1, 2]]); y = brn._policies(B[[1, 0, 1]])
    F = mon.solve(lists, x, y, C, THETA, max_sweeps=12)[0]
    for ch, reward in enumerate(((Pr > 0).astype(np.float64), (Pr < 0).astype(np.float64), np.ones(Pr.shape))):
        V = np.zeros(F[:, ch].shape)
        for _ in range(12):
            V = brn.sweep((Pp, Pn, reward, Pd), brn.EVAL_PAIR, x, y, V, C)[0]
        np.testing.assert_array_equal(bits(F[:, ch]), bits(V))


def test_row_0_is_not_read():
    lists, starts, A, B, r = game(0.2)
    A2 = A.copy(); B2 = B.copy()
    A2[:, 0] = np.nan; B2[:, 0] = [7.0, -3.0, 0.0, 1e300, 2.0]
    for cap in (1, 12):
        want = mon.match_outcomes(lists, starts, A[1:], B, C, THETA, max_sweeps=cap)
        got = mon.match_outcomes(lists, starts, A2[1:], B2, C, THETA, max_sweeps=cap)
        for k in want:
            np.testing.assert_array_equal(bits(got[k]) if k != "iterations" else got[k], bits(want[k]) if k != "iterations" else want[k])
        assert (got["values"][:, :, :, 0] == 0).all()


def test_a_pair_of_a_batch_has_the_bits_it_has_alone():
    lists, starts, A, B, r = game(0.2)
    it = r["iterations"].reshape(-1)
    lo, hi = int(it.argmin()), int(it.argmax())
    print("sweeps of the batch %s" % it.tolist())
    assert it[hi] - it[lo] > 16, "the batch should hold pairs whose sweep counts differ by more than 16"
    for flat in (lo, hi):
        alone = mon.match_outcomes(lists, starts, A, B, C, THETA, pairs=[flat])
        i, j = divmod(flat, 2)
        assert alone["iterations"][0] == it[flat]
        np.testing.assert_array_equal(bits(alone["values"][0]), bits(r["values"][i, j]))
        for name in mon.CHANNELS:
            np.testing.assert_array_equal(bits(alone[name][0]), bits(r[name][i, j]))
