"""The two-player solvers on the device at the edges of what they accept, on 5x4 at slips 0.0 and 0.2, bit for bit against the
numpy restatements over the CPU oracle's lists (tests/minimax_vi_np.py, tests/best_response_np.py, tests/cross_play_np.py):
both ends of discount_factor's [0, 1] and of theta's [0, +inf], the sweep cap either side of the 16 sweeps between two
synchronisations, minimax value iteration's iterate at a cap (RuntimeError.results), tied optima, policy rows that are accepted
but unusual (-0.0, subnormals, sums 9e-6 off 1) and the rows just past the rule, the limits of 256 policies and of 1024
policies a side run rather than refused, and a matrix that the library's own pairs_per_pass has to split.
tests/two_player_cases.py defines the cases; tests/test_two_player_edges_np.py shows, without a GPU, that each reaches its path."""
import os
import sys
import time

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_response_np as brn  # noqa: E402
import cross_play_np as cpn  # noqa: E402
import minimax_vi_np as mvn  # noqa: E402
from test_gpu_best_response import same_bits  # noqa: E402
from test_gpu_cross_play import kickoff_states, pairwise, policy_set, same_result  # noqa: E402
from test_matrix_game_host import build_games_host  # noqa: E402
from two_player_cases import (GAMMA0_TIED, INF, NS, PASS_GAMMA, PASS_NA, PASS_NB, PASS_PAIRS, PASS_SWEEPS, SLIPS,  # noqa: E402
                                      THETA, THETA0_CAPS, TIE_COUNTS, TIE_GAMMAS, UNDISCOUNTED_CAP, boundary_sample, edge_policies, in_chunks, odd_rows,
                                      pass_policies, pass_sample, pitch, refused_rows, restated_pairs, tied_states)

pytestmark = pytest.mark.gpu

W, H = 5, 4
NAMES = {4: ("br", "V", "Qr", "iterations"), 5: ("pi_a", "pi_b", "V", "Q")}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_games_host(tmp_path_factory.mktemp("games_gpu_edges"))


@pytest.fixture(scope="module")
def batch():
    """slip -> a handle, made once for this module"""
    made = {}

    def get(slip):
        if slip not in made:
            made[slip] = SoccerBatch(1, W, H, slip)
            assert made[slip].nS == NS and kickoff_states(made[slip]) == pitch(slip)[1]
        return made[slip]

    yield get
    for b in made.values():
        b.close()


def results(call):
    """(the tuple a solve returns or, stopped at its cap, carries in RuntimeError.results; whether it was stopped)"""
    try:
        return call(), False
    except RuntimeError as e:
        assert "without converging" in str(e) or "had not converged" in str(e)
        return e.results, True


def same_vi(got, want, what):
    """got: minimax_value_iteration's tuple; want: the restatement's (pi_a, pi_b, V, Q, k, capped)"""
    assert got[4] == want[4], "%s: %d sweeps, the restatement's %d" % (what, got[4], want[4])
    for name, x, y in zip(NAMES[5], got[:4], want[:4]):
        same_bits(x, y, "%s of %s" % (name, what))


def same_response(got, want, what):
    """(br, V, Qr, iterations) of a device call against the restatement's"""
    for name, x, y in zip(NAMES[4], got, want):
        same_bits(x, y, "%s of %s" % (name, what))


def all_modes(b, slip, pol, other, gamma, theta, cap, what):
    """best_response for both players on pol, evaluate_policies on (pol, other) and cross_play of pol x other with values, each
    against its restatement; returns {mode: (iterations, whether the device call was stopped at the cap)}"""
    lists, starts = pitch(slip)
    seen = {}
    for player in (0, 1):
        got, stopped = results(lambda: b.best_response(pol, player, theta, gamma, max_sweeps=cap))
        same_response(got, brn.best_response(lists, pol, player, gamma, theta, cap), "%s, response to player %s" % (what, "AB"[player]))
        seen["response_%d" % player] = (got[3], stopped)
    got, stopped = results(lambda: b.evaluate_policies(pol, other, theta, gamma, max_sweeps=cap))
    wV, wit = brn.evaluate(lists, pol, other, gamma, theta, cap)
    same_bits(got[0], wV, "V of %s, pairs" % what); same_bits(got[1], wit, "iterations of %s, pairs" % what)
    seen["pairs"] = (got[1], stopped)
    got, stopped = results(lambda: b.cross_play(pol, other, theta, gamma, max_sweeps=cap, values=True))
    same_result(got, cpn.cross_play(lists, starts, pol, other, gamma, theta, cap), "%s, cross-play" % what)
    seen["cross"] = (got[1], stopped)
    for it, stopped in seen.values():
        assert stopped == bool((it == cap).any())               # (no case here converges exactly at its cap)
    return seen


# ---- 1. the ends of discount_factor ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("slip", SLIPS)
def test_discount_0(slip, batch, host):
    b = batch(slip)
    lists, _ = pitch(slip)
    pol = edge_policies()
    got = b.minimax_value_iteration(THETA, 0.0)
    assert got[4] == 2
    same_vi(got, mvn.minimax_vi(host, lists, 0.0, THETA), "minimax value iteration at discount 0")
    seen = all_modes(b, slip, pol, np.roll(pol, 1, 0), 0.0, THETA, 1000000, "discount 0")
    assert all((it == 2).all() for it, _ in (seen["response_0"], seen["response_1"], seen["pairs"]))
    assert (seen["cross"][0] <= 2).all() and (seen["cross"][0] == 2).sum() >= 15
    for player in (0, 1):                                       # ties nearly everywhere: br is the first index
        br, V, Qr, it = b.best_response(pol, player, THETA, 0.0)
        assert tied_states(Qr, player).tolist() == [GAMMA0_TIED] * 4
        best = Qr.min(-1) if player == 0 else Qr.max(-1)
        np.testing.assert_array_equal(br, (Qr == best[..., None]).argmax(-1))


@pytest.mark.parametrize("slip", SLIPS)
def test_discount_1_under_a_cap_of_200(slip, batch, host):
    b = batch(slip)
    lists, _ = pitch(slip)
    pol = edge_policies()
    cap = UNDISCOUNTED_CAP
    seen = all_modes(b, slip, pol, pol, 1.0, THETA, cap, "discount 1")
    print("slip %.1f, discount 1, cap %d: %s" % (slip, cap, {k: v[0].tolist() for k, v in seen.items()}))
    for mode in ("response_0", "response_1", "cross"):          # one batch holds converged and capped members
        it = seen[mode][0]
        assert (it == cap).any() and (it < cap).any(), mode
    assert seen["response_0"][0][0] == {0.0: 111, 0.2: 159}[slip] and seen["response_0"][0][1] == cap
    # minimax value iteration: the restatement is still open at the cap on both slips
    want = mvn.minimax_vi(host, lists, 1.0, THETA, cap)
    assert want[5]
    got, stopped = results(lambda: b.minimax_value_iteration(THETA, 1.0, max_sweeps=cap))
    assert stopped
    same_vi(got, want, "minimax value iteration at discount 1, cap %d" % cap)


# ---- 2. the ends of theta ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slip", SLIPS)
def test_theta_inf_stops_at_sweep_1(slip, batch, host):
    b = batch(slip)
    lists, _ = pitch(slip)
    pol = edge_policies()
    got = b.minimax_value_iteration(INF, 0.9)
    assert got[4] == 1
    same_vi(got, mvn.minimax_vi(host, lists, 0.9, INF), "minimax value iteration at theta = inf")
    seen = all_modes(b, slip, pol, pol[::-1], 0.9, INF, 1000000, "theta = inf")
    assert all((it == 1).all() and not stopped for it, stopped in seen.values())


@pytest.mark.parametrize("cap", THETA0_CAPS)
@pytest.mark.parametrize("slip", SLIPS)
def test_theta_0_runs_to_the_cap(slip, cap, batch, host):
    b = batch(slip)
    lists, _ = pitch(slip)
    pol = edge_policies()
    got, stopped = results(lambda: b.minimax_value_iteration(0.0, 0.9, max_sweeps=cap))
    assert stopped and got[4] == cap
    same_vi(got, mvn.minimax_vi(host, lists, 0.9, 0.0, cap), "minimax value iteration at theta = 0, cap %d" % cap)
    seen = all_modes(b, slip, pol, pol[::-1], 0.9, 0.0, cap, "theta = 0, cap %d" % cap)
    assert all((it == cap).all() and stopped for it, stopped in seen.values())
    # a solve that reaches its fixed point exactly (discount 0: V_2 == V_1) still runs to the cap
    seen = all_modes(b, slip, pol, pol[::-1], 0.0, 0.0, cap, "theta = 0 at discount 0, cap %d" % cap)
    assert all((it == cap).all() and stopped for it, stopped in seen.values())


# ---- 3. minimax value iteration at a cap --------------------------------------------------------------------------------------
@pytest.mark.parametrize("slip", SLIPS)
def test_minimax_value_iteration_carries_its_iterate_at_a_cap(slip, batch, host):
    b = batch(slip)
    lists, _ = pitch(slip)
    gamma = 0.9
    full = mvn.minimax_vi(host, lists, gamma, THETA)
    k = full[4]
    same_vi(b.minimax_value_iteration(THETA, gamma), full, "the uncapped solve")
    caps = [k - 1, (k - 1) // 16 * 16, 1]
    assert caps[0] % 16 and caps[1] % 16 == 0 and 16 <= caps[1] < caps[0]
    at = {}
    for cap in caps:
        with pytest.raises(RuntimeError, match="stopped after max_sweeps = %d sweeps without converging" % cap) as e:
            b.minimax_value_iteration(THETA, gamma, max_sweeps=cap)
        at[cap] = e.value.results
        assert len(at[cap]) == 5 and at[cap][4] == cap
        want = mvn.minimax_vi(host, lists, gamma, THETA, cap)
        assert want[5]
        same_vi(at[cap], want, "minimax value iteration at a cap of %d" % cap)
    # V at a cap of k - 1 is V_{k-1}: one backup of it is the uncapped solve's sweep k
    pa, pb, V, Q, _ = b.minimax_backup(at[k - 1][2], gamma)
    same_vi((pa, pb, V, Q, k), full, "a backup of the iterate at k - 1")
    # a cap of k converges, and the capped calls left nothing behind
    same_vi(b.minimax_value_iteration(THETA, gamma, max_sweeps=k), full, "a cap of k")


# ---- 4. ties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", TIE_GAMMAS)
def test_tied_optima_take_the_first_index(gamma, batch):
    slip = 0.0
    b = batch(slip)
    lists, _ = pitch(slip)
    pol = edge_policies()
    for player in (0, 1):
        want = brn.best_response(lists, pol, player, gamma, THETA)
        ties = tied_states(want[2], player)
        print("slip 0, discount %.1f, response to player %s: tied states per policy %s" % (gamma, "AB"[player], ties.tolist()))
        assert (ties > 0).all() and ties.tolist() == TIE_COUNTS[(gamma, player)]
        same_response(b.best_response(pol, player, THETA, gamma), want, "the response to player %s with ties" % "AB"[player])


# ---- 5. policy rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slip", SLIPS)
def test_unusual_rows_are_solved_in_every_mode(slip, batch):
    pol = odd_rows()
    seen = all_modes(batch(slip), slip, pol, pol[::-1], 0.9, THETA, 1000000, "unusual rows")
    assert all(not stopped for _, stopped in seen.values())


def test_rows_just_past_the_rule_are_refused(batch):
    b = batch(0.2)
    for row, why in refused_rows():
        pol = np.full((3, NS, 5), 0.2)
        pol[1, 37] = row
        good = np.full((2, NS, 5), 0.2)
        for player in (0, 1):
            with pytest.raises(AssertionError, match=r"policy\[1\]\[37\] " + why):
                b.best_response(pol, player, THETA, 0.9)
        with pytest.raises(AssertionError, match=r"pi_a\[1\]\[37\] " + why):
            b.evaluate_policies(pol, np.full((3, NS, 5), 0.2), THETA, 0.9)
        with pytest.raises(AssertionError, match=r"pi_b\[1\]\[37\] " + why):
            b.evaluate_policies(np.full((3, NS, 5), 0.2), pol, THETA, 0.9)
        with pytest.raises(AssertionError, match=r"pi_a\[1\]\[37\] " + why):
            b.cross_play(pol, good, THETA, 0.9)
        with pytest.raises(AssertionError, match=r"pi_b\[1\]\[37\] " + why):
            b.cross_play(good, pol, THETA, 0.9)


# ---- 6. the limits, run ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slip", SLIPS)
def test_256_policies(slip, batch):
    b = batch(slip)
    lists, _ = pitch(slip)
    gamma = 0.5
    pol = policy_set(W, H, slip, 256, 51)
    other = policy_set(W, H, slip, 256, 52)
    for player in (0, 1):
        got = b.best_response(pol, player, THETA, gamma)
        want = in_chunks(lambda p: brn.best_response(lists, p, player, gamma, THETA), pol)
        same_response(got, want, "256 responses to player %s" % "AB"[player])
        assert len(set(got[3].tolist())) > 2
        for i in (0, 127, 255):
            alone = b.best_response(pol[i], player, THETA, gamma)
            for name, x, y in zip(NAMES[4][:3], got, alone):
                same_bits(x[i], y, "%s of member %d alone" % (name, i))
            assert got[3][i] == alone[3]
    V, it = b.evaluate_policies(pol, other, THETA, gamma)
    wV, wit = in_chunks(lambda p, q: brn.evaluate(lists, p, q, gamma, THETA), pol, other)
    same_bits(V, wV, "V of 256 pairs"); same_bits(it, wit, "iterations of 256 pairs")
    for i in (0, 127, 255):
        Vi, ki = b.evaluate_policies(pol[i], other[i], THETA, gamma)
        same_bits(V[i], Vi, "V of pair %d alone" % i)
        assert it[i] == ki


@pytest.mark.parametrize("n_a,n_b", [(1024, 1), (1, 1024), (1024, 2)])
@pytest.mark.parametrize("slip", SLIPS)
def test_1024_policies_a_side(slip, n_a, n_b, batch):
    b = batch(slip)
    gamma = 0.5
    A = policy_set(W, H, slip, n_a, 53)
    B = policy_set(W, H, slip, n_b, 54)
    got = b.cross_play(A, B, THETA, gamma, values=True)
    assert got[0].shape == (n_a, n_b)
    same_result(got, pairwise(b, A, B, theta=THETA, gamma=gamma), "%d x %d" % (n_a, n_b))
    flat = boundary_sample(n_a * n_b)
    assert len(flat) >= 32
    want = restated_pairs(slip, A, B, flat, gamma, THETA)
    same_result([x.reshape((n_a * n_b,) + x.shape[2:])[flat] for x in got], want, "the sampled pairs of %d x %d" % (n_a, n_b))
    assert len(set(got[1].reshape(-1).tolist())) > 2


# ---- 7. the library's own pass split --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slip", SLIPS)
def test_the_library_s_own_choice_splits_a_matrix_above_one_pass(slip, batch):
    b = batch(slip)
    A, B = pass_policies()
    total = PASS_NA * PASS_NB
    assert total == 89088 > PASS_PAIRS == 88128
    t0 = time.perf_counter()
    own = b.cross_play(A, B, THETA, PASS_GAMMA, pairs_per_pass=0, values=True)
    t1 = time.perf_counter()
    assert own[1].max() <= PASS_SWEEPS
    cut = b.cross_play(A, B, THETA, PASS_GAMMA, pairs_per_pass=1024, values=True)
    t2 = time.perf_counter()
    same_result(own, cut, "1024 x 87 in the library's passes, against passes of 1024")
    del cut
    bare = b.cross_play(A, B, THETA, PASS_GAMMA, pairs_per_pass=0)
    t3 = time.perf_counter()
    print("slip %.1f, 1024 x 87 at discount %.2f: sweeps %d .. %d; the library's passes with values %.2f s, passes of 1024 %.2f s, "
          "the library's without values %.2f s" % (slip, PASS_GAMMA, own[1].min(), own[1].max(), t1 - t0, t2 - t1, t3 - t2))
    assert len(bare) == 2
    same_result(bare, own[:2], "1024 x 87 without values")
    flat = pass_sample()
    assert len(flat) >= 32 and {PASS_PAIRS - 1, PASS_PAIRS, total - 1} <= set(flat)
    want = restated_pairs(slip, A, B, flat, PASS_GAMMA, THETA)
    same_result([x.reshape((total,) + x.shape[2:])[flat] for x in own], want, "the sampled pairs of 1024 x 87")
