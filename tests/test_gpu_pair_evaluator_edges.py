"""The pair evaluators on the device (soccer_match_outcomes, soccer_occupancy, soccer_policy_gradient, soccer_gradient_play_*) at
the edges of what they accept, on 5x4 at slips 0.0 and 0.2, bit for bit against the numpy restatements over the CPU oracle's
lists (tests/match_outcomes_np.py, tests/occupancy_np.py, tests/policy_gradient_np.py), the iterates carried in
RuntimeError.results at a cap included: both ends of continue_prob / discount_factor's [0, 1] and of theta's [0, +inf], the sweep
cap either side of the 16 sweeps between two synchronisations, policy rows that are accepted but unusual (-0.0, subnormals, sums
9e-6 off 1) and the rows just past the rule, the limit of 1024 policies a side run rather than refused, columns of the policy
gradient that span passes, and for each call a matrix that its own pairs_per_pass has to split.
tests/pair_evaluator_cases.py defines the cases; tests/test_pair_evaluator_cases_np.py shows, without a GPU, that each reaches
its path."""
import os
import sys
import time

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occupancy_np as ocn  # noqa: E402
import pair_evaluator_cases as pc  # noqa: E402
import policy_gradient_np as pgn  # noqa: E402
from test_gpu_best_response import same_bits  # noqa: E402
from test_gpu_cross_play import kickoff_states  # noqa: E402
from test_gpu_policy_gradient import PAIR_KEYS, SUM_KEYS, same_state  # noqa: E402
from two_player_cases import (INF, NS, SLIPS, THETA, THETA0_CAPS, UNDISCOUNTED_CAP, boundary_sample, edge_policies, odd_rows,  # noqa: E402
                              pitch, refused_rows)

pytestmark = pytest.mark.gpu

W, H = 5, 4
F = pc.features_of(NS)
KEYS = {"match": ("win_a", "win_b", "length", "iterations", "values"), "occupancy": ("length", "expect", "iterations", "occupancy"),
        "gradient": PAIR_KEYS + SUM_KEYS}
BARE = {"match": KEYS["match"][:4], "occupancy": KEYS["occupancy"][:3], "gradient": ("payoff", "iterations")}


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


def capped(call):
    """(the dict a call returns or, stopped at its cap, carries in RuntimeError.results; the error's message or None)"""
    try:
        return call(), None
    except RuntimeError as e:
        return e.results, str(e)


def device(b, call, A, B, c, theta, cap=1000000, values=True, **kw):
    """one of the three calls with everything asked for; the policy gradient under the cases' weights and normalize=True"""
    if call == "match":
        return b.match_outcomes(A, B, theta, c, max_sweeps=cap, values=values, **kw)
    if call == "occupancy":
        return b.occupancy(A, B, theta, c, features=F, values=values, max_sweeps=cap, **kw)
    return b.policy_gradient(A, B, theta, c, w_a=pc.weights(len(A)), w_b=pc.weights(len(B)), normalize=True, values=values,
                             max_sweeps=cap, **kw)


def all_calls(b, slip, name, A, B, c, theta, cap=1000000):
    """the three calls on A x B, each against its restatement on everything it returns, also where it stops at the cap; returns
    ({"match", "occupancy", "V", "D"}: the device's sweep counts, {call: whether it was stopped}, {call: what it returned})"""
    want = pc.three_calls(name, slip, A, B, c, theta, cap)
    total = len(A) * len(B)
    seen, stopped = {}, {}
    for call in pc.CALLS:
        what = "%s of %s at c = %g, theta = %g, cap %d" % (call, name, c, theta, cap)
        got, msg = capped(lambda: device(b, call, A, B, c, theta, cap))
        for k in KEYS[call]:
            same_bits(got[k], want[call][k], "%s of %s" % (k, what))
        it = want[call]["iterations"]
        open_pairs = (it == cap).any(-1) if call == "gradient" else it == cap       # (no solve here converges exactly at its cap)
        if open_pairs.any():
            assert msg is not None and "%d of %d pairs had not converged after max_sweeps = %d" % (open_pairs.sum(), total, cap) in msg, (what, msg)
        else:
            assert msg is None, (what, msg)
        stopped[call] = msg is not None
        seen[call] = got
    return pc.counts(seen), stopped, seen


def edge_pair():
    pol = edge_policies()
    return pol, np.roll(pol, 1, 0)


# ---- 1. the ends of continue_prob / discount_factor ----------------------------------------------------------------------------
@pytest.mark.parametrize("slip", SLIPS)
def test_continue_prob_0(slip, batch):
    b = batch(slip)
    A, B = edge_pair()
    k, stopped, got = all_calls(b, slip, "edge", A, B, 0.0, THETA)
    assert not any(stopped.values())
    assert (k["match"] == 2).all() and (k["occupancy"] == 2).all() and (k["D"] == 2).all()
    assert set(k["V"].reshape(-1).tolist()) == ({1, 2} if slip == 0.0 else {2})
    # a game of exactly one step, played from the kick-off states
    mu = ocn.start_distribution(NS, pitch(slip)[1])
    # (length is 1.0 to the bit where both rows are one-hot and nothing slips, the restatement's rounding of 1.0 elsewhere)
    L = got["match"]["length"]
    assert (slip != 0.0 or (L[2:, [0, 3]] == 1.0).all()) and np.abs(L - 1.0).max() <= 405 * 2.0 ** -53
    same_bits(b.occupancy(A, B, THETA, 0.0, values=True)["occupancy"], np.broadcast_to(mu, (4, 4, NS)), "the occupancy at continue_prob 0")
    same_bits(b.policy_gradient(A, B, THETA, 0.0, values=True)["occupancy"], np.broadcast_to(mu, (4, 4, NS)), "the policy gradient's D at discount 0")


@pytest.mark.parametrize("slip", SLIPS)
def test_continue_prob_1_under_a_cap_of_200(slip, batch):
    b = batch(slip)
    A, B = edge_pair()
    cap = UNDISCOUNTED_CAP
    k, stopped, got = all_calls(b, slip, "edge", A, B, 1.0, THETA, cap)
    print("slip %.1f, continue_prob 1, cap %d: V sweeps %s" % (slip, cap, k["V"].reshape(-1).tolist()))
    assert all(stopped.values())
    assert (k["match"] == cap).all() and (k["occupancy"] == cap).all() and (k["D"] == cap).all()
    # the policy gradient holds converged and capped V solves side by side; its sums are those of the last iterates
    assert int((k["V"] == cap).sum()) == {0.0: 11, 0.2: 14}[slip] and (k["V"] < cap).any()
    got = got["gradient"]
    sums = pgn.reduce(got["occupancy"], got["q_a"], got["q_b"], pc.weights(4), pc.weights(4), True)
    for name, s in zip(SUM_KEYS, sums):
        same_bits(got[name], s, "%s at the cap from the last iterates" % name)


# ---- 2. the ends of theta ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slip", SLIPS)
def test_theta_inf_stops_at_sweep_1(slip, batch):
    A, B = edge_pair()
    k, stopped, got = all_calls(batch(slip), slip, "edge", A, B, 0.9, INF)
    assert all((v == 1).all() for v in k.values()) and not any(stopped.values())


@pytest.mark.parametrize("cap", THETA0_CAPS)
@pytest.mark.parametrize("slip", SLIPS)
def test_theta_0_runs_to_the_cap(slip, cap, batch):
    A, B = edge_pair()
    for c in (0.9, 0.0):                                        # (at 0 the fixed point is reached exactly at sweep 2)
        k, stopped, got = all_calls(batch(slip), slip, "edge", A, B, c, 0.0, cap)
        assert all((v == cap).all() for v in k.values()) and all(stopped.values()), c


# ---- 3. policy rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slip", SLIPS)
def test_unusual_rows_are_solved_in_every_call(slip, batch):
    b = batch(slip)
    pol = odd_rows()
    k, stopped, got = all_calls(b, slip, "odd", pol, pol[::-1], 0.9, THETA)
    assert not any(stopped.values()) and all((v > 100).all() and (v < pc.UNUSUAL_SWEEPS).all() for v in k.values())
    # two steps of gradient play from them: the projection meets -0.0, subnormals and rows 9e-6 off the simplex
    lists, starts = pitch(slip)
    x, y, prev_a, prev_b, trace = pgn.gradient_play(lists, starts, pol, pol[::-1], 2, 0.9, THETA, inl=pc.in_lists(slip), **pc.PLAY)
    g = b.gradient_play(n_a=2, n_b=2, discount_factor=0.9, theta=THETA, pi_a=pol, pi_b=pol[::-1], **pc.PLAY)
    same_bits(g.run(2, trace=True), trace, "the trace of two steps from the unusual rows")
    r = g.read()
    same_state(r, x, y, prev_a, prev_b, 2, "after two steps from the unusual rows")
    assert np.isfinite(r["pi_a"]).all() and (r["pi_a"] >= 0).all() and np.abs(r["pi_a"][:, 1:].sum(2) - 1).max() < 1e-14
    g.close()


def test_rows_just_past_the_rule_are_refused(batch):
    b = batch(0.2)
    good = np.full((2, NS, 5), 0.2)
    for row, why in refused_rows():
        pol = np.full((3, NS, 5), 0.2)
        pol[1, 37] = row
        for call, name in (("match", "soccer_match_outcomes"), ("occupancy", "soccer_occupancy"), ("gradient", "soccer_policy_gradient")):
            with pytest.raises(AssertionError, match=name + r": pi_a\[1\]\[37\].*" + why):
                device(b, call, pol, good, 0.9, THETA)
            with pytest.raises(AssertionError, match=name + r": pi_b\[1\]\[37\].*" + why):
                device(b, call, good, pol, 0.9, THETA)
        with pytest.raises(AssertionError, match=r"soccer_gradient_play_create: pi_a\[1\]\[37\].*" + why):
            b.gradient_play(n_a=3, pi_a=pol)
        with pytest.raises(AssertionError, match=r"soccer_gradient_play_create: pi_b\[1\]\[37\].*" + why):
            b.gradient_play(n_b=3, pi_b=pol)


# ---- 4. the limit of 1024 policies a side, run ------------------------------------------------------------------------------------
def three_pairs(n_a, n_b):
    total = n_a * n_b
    return [divmod(f, n_b) for f in (0, total // 2, total - 1)]


@pytest.mark.parametrize("call", ["match", "occupancy"])
@pytest.mark.parametrize("n_a,n_b", pc.LIMIT_SHAPES)
@pytest.mark.parametrize("slip", SLIPS)
def test_1024_policies_a_side(slip, n_a, n_b, call, batch):
    b = batch(slip)
    A, B = pc.limit_policies(n_a, n_b)
    total = n_a * n_b
    got = device(b, call, A, B, pc.LIMIT_C, THETA, values=False)
    assert got["length"].shape == (n_a, n_b) and sorted(k for k in got if k in KEYS[call]) == sorted(BARE[call])
    flat = boundary_sample(total)
    assert len(flat) >= 32
    want = pc.restate(call, slip, A, B, pc.LIMIT_C, THETA, pairs=flat)
    for k in BARE[call]:
        same_bits(got[k].reshape((total,) + got[k].shape[2:])[flat], want[k], "%s of the sampled pairs of %d x %d" % (k, n_a, n_b))
    for i, j in three_pairs(n_a, n_b):
        alone = device(b, call, A[i], B[j], pc.LIMIT_C, THETA, values=False)
        for k in BARE[call]:
            same_bits(got[k][i, j], alone[k][0, 0], "%s of pair (%d, %d) alone" % (k, i, j))
    assert got["iterations"].max() <= 36                        # (match outcomes' length channel keeps every pair at 34 or 35)


@pytest.mark.parametrize("n_a,n_b", pc.LIMIT_SHAPES)
@pytest.mark.parametrize("slip", SLIPS)
def test_1024_policies_a_side_in_the_policy_gradient(slip, n_a, n_b, batch):
    b = batch(slip)
    A, B = pc.limit_policies(n_a, n_b)
    total = n_a * n_b
    got = b.policy_gradient(A, B, THETA, pc.LIMIT_C)
    assert got["payoff"].shape == (n_a, n_b) and got["grad_a"].shape == (n_a, NS, 5) and got["grad_b"].shape == (n_b, NS, 5)
    flat = boundary_sample(total)
    want = pc.restate("gradient", slip, A, B, pc.LIMIT_C, THETA, pairs=flat)
    same_bits(got["payoff"].reshape(-1)[flat], want["payoff"], "payoff of the sampled pairs of %d x %d" % (n_a, n_b))
    same_bits(got["iterations"].reshape(total, 2)[flat], want["iterations"], "iterations of the sampled pairs of %d x %d" % (n_a, n_b))
    for i, j in three_pairs(n_a, n_b):
        alone = b.policy_gradient(A[i], B[j], THETA, pc.LIMIT_C)
        same_bits(got["payoff"][i, j], alone["payoff"][0, 0], "payoff of pair (%d, %d) alone" % (i, j))
        same_bits(got["iterations"][i, j], alone["iterations"][0, 0], "iterations of pair (%d, %d) alone" % (i, j))
        # against a single opponent (weight 1.0) a policy's sums are its one pair's
        if n_b == 1:
            same_bits(got["grad_a"][i], alone["grad_a"][0], "grad_a[%d] alone" % i); same_bits(got["reach_a"][i], alone["reach_a"][0], "reach_a[%d] alone" % i)
        if n_a == 1:
            same_bits(got["grad_b"][j], alone["grad_b"][0], "grad_b[%d] alone" % j); same_bits(got["reach_b"][j], alone["reach_b"][0], "reach_b[%d] alone" % j)
    assert got["iterations"].max() <= 36 and np.isfinite(got["grad_a"]).all() and np.isfinite(got["grad_b"]).all()


@pytest.mark.parametrize("slip", SLIPS)
def test_columns_of_the_policy_gradient_that_span_passes(slip, batch):
    b = batch(slip)
    n_a, n_b = pc.SPAN_SHAPE
    A, B = pc.limit_policies(n_a, n_b)
    w_a, w_b = pc.weights(n_a), pc.weights(n_b)
    one = device(b, "gradient", A, B, pc.LIMIT_C, THETA)
    for per in pc.SPAN_PASSES:
        got = device(b, "gradient", A, B, pc.LIMIT_C, THETA, pairs_per_pass=per)
        for k in KEYS["gradient"]:
            same_bits(got[k], one[k], "%s of 67 x 7 in passes of %d against one pass" % (k, per))
        for name, s in zip(SUM_KEYS, pgn.reduce(got["occupancy"], got["q_a"], got["q_b"], w_a, w_b, True)):
            same_bits(got[name], s, "%s of 67 x 7 in passes of %d from its pairs" % (name, per))
    flat = boundary_sample(n_a * n_b)
    want = pc.restate("gradient", slip, A, B, pc.LIMIT_C, THETA, pairs=flat)
    same_bits(one["payoff"].reshape(-1)[flat], want["payoff"], "payoff of the sampled pairs of 67 x 7")
    same_bits(one["iterations"].reshape(-1, 2)[flat], want["iterations"], "iterations of the sampled pairs of 67 x 7")


@pytest.mark.parametrize("slip", SLIPS)
def test_gradient_play_of_1024_policies_against_one(slip, batch):
    b = batch(slip)
    A, B = pc.limit_policies(1024, 1)
    theta = 1e-8
    g = b.gradient_play(n_a=1024, n_b=1, discount_factor=pc.LIMIT_C, theta=theta, pi_a=A, pi_b=B, **pc.PLAY)
    got = g.run(2, trace=True)
    x, y, prev_a, prev_b, trace = A, B, np.zeros(A.shape), np.zeros(B.shape), []
    for t in range(2):
        r = b.policy_gradient(x, y, theta, pc.LIMIT_C, normalize=True)
        trace.append(r["payoff"])
        x, y, prev_a, prev_b = pgn.step(x, y, r["grad_a"], r["grad_b"], prev_a, prev_b, t == 0, pc.PLAY["eta_a"], pc.PLAY["eta_b"],
                                        pc.PLAY["optimism"])
    same_bits(got, np.stack(trace), "the trace of two steps")
    same_state(g.read(), x, y, prev_a, prev_b, 2, "after two steps of 1024 x 1")
    g.close()


# ---- 5. the library's own pass split --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", pc.CALLS)
@pytest.mark.parametrize("slip", SLIPS)
def test_the_library_s_own_choice_splits_a_matrix_above_one_pass(slip, call, batch):
    b = batch(slip)
    A, B = pc.pass_matrix(call)
    n_b = len(B)
    per, total = pc.PASS_PAIRS[call], 1024 * n_b
    assert per < total
    values = call != "gradient"                                 # (the policy gradient's q_a and q_b would be 400 MB each and more)
    t0 = time.perf_counter()
    own = device(b, call, A, B, pc.PASS_C, THETA, values=values, pairs_per_pass=0)
    own.pop("visit_share", None)
    t1 = time.perf_counter()
    assert own["iterations"].max() <= pc.PASS_SWEEPS
    cut = device(b, call, A, B, pc.PASS_C, THETA, values=values, pairs_per_pass=1024)
    cut.pop("visit_share", None)
    t2 = time.perf_counter()
    print("slip %.1f, %s of 1024 x %d at %.2f: sweeps %d .. %d; the library's passes %.2f s, passes of 1024 %.2f s" % (
        slip, call, n_b, pc.PASS_C, own["iterations"].min(), own["iterations"].max(), t1 - t0, t2 - t1))
    assert sorted(own) == sorted(cut)
    for k in own:
        same_bits(own[k], cut[k], "%s of 1024 x %d in the library's passes, against passes of 1024" % (k, n_b))
    del cut
    flat = pc.pass_sample(call)
    assert {0, per - 1, per, total - 1} <= set(flat)
    want = pc.restate(call, slip, A, B, pc.PASS_C, THETA, pairs=flat)
    for k in (KEYS if values else BARE)[call]:
        same_bits(own[k].reshape((total,) + own[k].shape[2:])[flat], want[k], "%s of the sampled pairs of 1024 x %d" % (k, n_b))
    if call != "gradient":
        return
    # the running sums carried over the boundary, which lies inside row 964: that row's sums from a call on the row alone, and
    # the first and the last column's from calls on the column alone
    w_a, w_b = pc.weights(1024), pc.weights(n_b)
    i, j0 = divmod(per, n_b)
    assert 0 < j0 < n_b
    row = b.policy_gradient(A[i:i + 1], B, THETA, pc.PASS_C, w_b=w_b, normalize=True, values=True)
    ga, _, ra, _ = pgn.reduce(row["occupancy"], row["q_a"], row["q_b"], None, w_b, True)
    same_bits(own["grad_a"][i], ga[0], "grad_a of the row that straddles the boundary"); same_bits(own["reach_a"][i], ra[0], "... and its reach_a")
    for j in (0, n_b - 1):
        col = b.policy_gradient(A, B[j:j + 1], THETA, pc.PASS_C, w_a=w_a, normalize=True, values=True)
        _, gb, _, rb = pgn.reduce(col["occupancy"], col["q_a"], col["q_b"], w_a, None, True)
        same_bits(own["grad_b"][j], gb[0], "grad_b of column %d" % j); same_bits(own["reach_b"][j], rb[0], "reach_b of column %d" % j)
