"""Match outcomes on the device (soccer_match_outcomes): every sampled pair to the bits and the sweep count of the numpy
restatement (tests/match_outcomes_np.py) on every matrix shape; per-lane stopping inside a wave; no result depends on how the
matrix is cut into passes, on what the handle's buffers held before or on whether the values are asked for; the sweep cap; the
win margin against cross-play's payoff; the refusals; the populations; and a large pitch."""
import os
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch, SoccerSimultaneousEnv, VectorSoccerEnv
from gym_soccer_littman94_amd import planners as pl
from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_response_np as brn  # noqa: E402
import cross_play_np as cpn  # noqa: E402
import match_outcomes_np as mon  # noqa: E402
from test_gpu_best_response import oracle_lists, same_bits  # noqa: E402
from test_gpu_cross_play import kickoff_states, policy_set  # noqa: E402

pytestmark = pytest.mark.gpu

C, THETA = 0.9, 1e-10
PITCHES = [(5, 4, 0.0), (5, 4, 0.2), (7, 5, 0.3)]
# the continuation probability per pitch: 0.9 takes some 200 sweeps, which the restatement affords on 761 states; on 7x5's 2 381
# it would take minutes, and 0.5 (no channel moves by more than 0.5^(k-1) in sweep k: at most 35 sweeps) shows the same bits
C_OF = {(5, 4, 0.0): C, (5, 4, 0.2): C, (7, 5, 0.3): 0.5}
SHAPES = [(1, 1), (3, 5), (64, 2), (7, 67)]
NA, NB = 64, 67                                     # every shape is a corner of one NA x NB matrix of policies
MARGIN = 3 * C * THETA / (1 - C)                    # three fixed points of one modulus, each stopped at theta
CONSERVED = (2 * C + (1 - C)) * C * THETA / (1 - C)
KEYS = ("win_a", "win_b", "length", "iterations", "values")
# the pairs (i, j) that are restated, 12 of them.  Of the 7 x 67 matrix's 469: the first, 63 and 64 either side of the first
# wave's end, and every 117th (117 = 9 * 13 is coprime to 64) up to the last, 468 = 4 * 117 — 7 pairs; of 3 x 5 two more, its
# last among them; of 64 x 2 its pairs 63 and 64 either side of the wave's end and its last
SAMPLE = sorted({divmod(f, 67) for f in (0, 63, 64, 117, 234, 351, 468)} | {(1, 2), (2, 4)} | {(31, 1), (32, 0), (63, 1)})

_want, _full = {}, {}


def sets(w, h, slip, n_a=NA, n_b=NB):
    """test_gpu_cross_play's policy sets; a smaller set is the head of a larger one"""
    return policy_set(w, h, slip, NA, 31)[:n_a], policy_set(w, h, slip, NB, 32)[:n_b]


def starts_of(w, h, slip):
    return cpn.isd_obs(Oracle(w, h, slip, n=1, seed=0))


def restated(w, h, slip):
    """{(i, j): the restatement's dict of that pair} for the pairs of SAMPLE, computed once per pitch"""
    if (w, h, slip) not in _want:
        A, B = sets(w, h, slip)
        r = mon.match_outcomes(oracle_lists(w, h, slip), starts_of(w, h, slip), A, B, C_OF[(w, h, slip)], THETA,
                               pairs=[i * NB + j for i, j in SAMPLE])
        _want[(w, h, slip)] = {ij: {k: r[k][n] for k in KEYS} for n, ij in enumerate(SAMPLE)}
    return _want[(w, h, slip)]


def full_7x67(w, h, slip):
    """(A, B, the uncapped 7 x 67 result with values) on a handle of its own, computed once"""
    if (w, h, slip) not in _full:
        A, B = sets(w, h, slip, 7, 67)
        b = SoccerBatch(1, w, h, slip)
        _full[(w, h, slip)] = (A, B, b.match_outcomes(A, B, THETA, C, values=True))
        b.close()
    return _full[(w, h, slip)]


def same_result(got, want, what, keys=None):
    if keys is None:
        assert sorted(got) == sorted(want), (sorted(got), sorted(want))
        keys = sorted(want)
    for k in keys:
        same_bits(got[k], want[k], "%s of %s" % (k, what))


def derived(r):
    """draw and games_per_step are what the dict says they are"""
    same_bits(r["draw"], 1.0 - r["win_a"] - r["win_b"], "draw")
    same_bits(r["games_per_step"], 1.0 / r["length"], "games_per_step")
    assert r["iterations"].dtype == np.int64


def noop(nS):
    return brn.onehot(np.zeros(nS, np.int64))


# ---- 1. every shape against the restatement, and per-lane stopping -----------------------------------------------------------
@pytest.mark.parametrize("w,h,slip", PITCHES)
def test_sampled_pairs_of_every_shape_are_the_restatement_s_bits(w, h, slip):
    want, c = restated(w, h, slip), C_OF[(w, h, slip)]
    b = SoccerBatch(1, w, h, slip)
    assert kickoff_states(b) == starts_of(w, h, slip)
    for n_a, n_b in SHAPES:
        A, B = sets(w, h, slip, n_a, n_b)
        got = b.match_outcomes(A, B, THETA, c, values=True)
        assert sorted(got) == ["draw", "games_per_step", "iterations", "length", "values", "win_a", "win_b"]
        assert all(got[k].shape == (n_a, n_b) for k in got if k != "values") and got["values"].shape == (n_a, n_b, 3, b.nS)
        derived(got)
        inside = [(i, j) for i, j in SAMPLE if i < n_a and j < n_b]
        print("%dx%d slip %.1f, %d x %d: %d of %d pairs restated" % (w, h, slip, n_a, n_b, len(inside), n_a * n_b))
        assert (0, 0) in inside and (n_a - 1, n_b - 1) in inside
        for i, j in inside:
            for k in KEYS:
                same_bits(got[k][i, j], want[(i, j)][k], "%s of pair (%d, %d) of %d x %d" % (k, i, j, n_a, n_b))
        assert (got["values"][:, :, :, 0] == 0).all()
        assert (got["values"] >= 0).all() and (got["length"] >= 1.0 - 1e-12).all() and (got["draw"] > 0).all()
    # (the last shape is 7 x 67) per-lane stopping: within one wave of 64 pairs the sweep counts are more than a full host
    # batch of 16 apart, and the pair index i changes inside a wave
    assert (n_a, n_b) == (7, 67) and len(inside) == 9                       # (3 x 5's two lie in it as well)
    it = got["iterations"].reshape(-1)
    spread = [int(it[p:p + 64].max() - it[p:p + 64].min()) for p in range(0, it.size, 64)]
    print("%dx%d slip %.1f, 7 x 67 at c = %.1f: sweeps %d .. %d, spread per wave of 64 pairs %s" % (w, h, slip, c, it.min(), it.max(), spread))
    assert len(spread) == 8 and (max(spread) > 16 or c != C)
    # a single [nS, 5] policy is a batch of one
    one = b.match_outcomes(A[2], B[5], THETA, c, values=True)
    assert one["win_a"].shape == (1, 1)
    same_result(one, {k: got[k][2:3, 5:6] for k in got}, "a single pair")
    b.close()


# ---- 2. passes and cached buffers -------------------------------------------------------------------------------------------
def test_no_result_depends_on_the_passes_or_on_what_the_buffers_held():
    w, h, slip = 5, 4, 0.2
    A, B, want = full_7x67(w, h, slip)
    b = SoccerBatch(1, w, h, slip)
    small_first = b.match_outcomes(A[:3], B[:5], THETA, C, values=True)        # (buffers for 64 pairs, regrown below)
    for ppp in (64, 128, 448, 0):
        same_result(b.match_outcomes(A, B, THETA, C, pairs_per_pass=ppp, values=True), want, "7 x 67 with pairs_per_pass = %d" % ppp)
    same_result(b.match_outcomes(A[:3], B[:5], THETA, C, values=True), small_first, "3 x 5 after 7 x 67, against a fresh handle's")
    same_result(small_first, {k: want[k][:3, :5] for k in want}, "3 x 5 as a corner of 7 x 67")
    # after a call that failed: at the cap, and refused
    with pytest.raises(RuntimeError, match="469 of 469 pairs had not converged after max_sweeps = 3"):
        b.match_outcomes(A, B, THETA, C, max_sweeps=3, pairs_per_pass=128)
    with pytest.raises(AssertionError, match="pairs_per_pass"):
        b.match_outcomes(A, B, THETA, C, pairs_per_pass=63)
    same_result(b.match_outcomes(A, B, THETA, C, pairs_per_pass=64, values=True), want, "7 x 67 after two failed calls")
    b.close()


# ---- 3. the values are an extra ---------------------------------------------------------------------------------------------
def test_the_other_outputs_do_not_depend_on_whether_the_values_are_asked_for():
    w, h, slip = 5, 4, 0.2
    A, B, want = full_7x67(w, h, slip)
    b = SoccerBatch(1, w, h, slip)
    got = b.match_outcomes(A, B, THETA, C)
    assert "values" not in got and len(got) == 6
    same_result(got, want, "7 x 67 without values", keys=sorted(got))
    assert (want["values"][:, :, 0, 0] == 0).all() and (want["values"][:, :, :, 0] == 0).all()
    # the kick-off numbers are the values' mean over the initial states in their order
    for ch, name in enumerate(mon.CHANNELS):
        same_bits(want[name], cpn.kickoff(want["values"][:, :, ch], kickoff_states(b)), name + " from the values")
    b.close()


# ---- 4. the sweep cap -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta", [THETA, 0.2])
def test_the_sweep_cap_marks_the_open_pairs_and_keeps_their_last_iterate(theta):
    """theta = 1e-10 leaves every pair open at these caps; at theta = 0.2 no channel moves by more than 0.9^(k-1), below 0.2
    from k = 17 on, so the pairs stop at 17 sweeps or a few earlier: the caps of 16 and 17 meet pairs of both kinds"""
    w, h, slip = 5, 4, 0.2
    A, B = sets(w, h, slip, 3, 5)
    lists, starts = oracle_lists(w, h, slip), starts_of(w, h, slip)
    # each pair's sweeps, as far as the caps ask: a pair still open after 34 is open at every cap
    free = mon.match_outcomes(lists, starts, A, B, C, theta, max_sweeps=34)["iterations"]
    print("theta %g: sweeps of the 3 x 5 pairs, 34 for more\n%s" % (theta, free))
    b = SoccerBatch(1, w, h, slip)
    mixed = 0
    for cap in (1, 16, 17, 33):
        want = mon.match_outcomes(lists, starts, A, B, C, theta, max_sweeps=cap)
        late = free > cap
        if not late.any():
            got = b.match_outcomes(A, B, theta, C, max_sweeps=cap, values=True)
        else:
            with pytest.raises(RuntimeError, match="%d of 15 pairs had not converged after max_sweeps = %d" % (late.sum(), cap)) as e:
                b.match_outcomes(A, B, theta, C, max_sweeps=cap, values=True)
            got = e.value.results
        mixed += bool(late.any() and (~late).any())
        same_bits(got["iterations"], np.where(late, cap, free), "iterations at a cap of %d" % cap)
        same_result(got, want, "the 3 x 5 matrix at a cap of %d" % cap, keys=KEYS)
        derived(got)
    assert mixed >= 1 if theta == 0.2 else (free > 33).all()
    b.close()


def test_a_pair_that_never_moves_plays_exactly_max_sweeps_steps():
    b = SoccerBatch(1, 5, 4, 0.0)
    for cap in (1, 16, 17, 33):
        with pytest.raises(RuntimeError, match="1 of 1 pairs had not converged") as e:
            b.match_outcomes(noop(b.nS), noop(b.nS), THETA, 1.0, max_sweeps=cap, values=True)
        r = e.value.results
        assert r["length"][0, 0] == float(cap) and r["iterations"][0, 0] == cap and r["win_a"][0, 0] == 0 and r["win_b"][0, 0] == 0
        assert (r["values"][0, 0, 2, 1:] == float(cap)).all() and (r["values"][0, 0, :2] == 0).all() and r["draw"][0, 0] == 1.0
    b.close()


# ---- 5. against cross-play ----------------------------------------------------------------------------------------------------
def test_the_win_margin_is_cross_play_s_payoff_and_the_outcomes_add_up():
    w, h, slip = 5, 4, 0.2
    A, B, r = full_7x67(w, h, slip)
    b = SoccerBatch(1, w, h, slip)
    payoff = b.cross_play(A, B, THETA, C)[0]
    b.close()
    err = np.abs((r["win_a"] - r["win_b"]) - payoff).max()
    cons = np.abs(C * (r["win_a"] + r["win_b"]) + (1 - C) * r["length"] - 1.0).max()
    print("max |(win_a - win_b) - payoff| %.3g (bound %.3g), conservation %.3g (bound %.3g)" % (err, MARGIN, cons, CONSERVED))
    assert err <= MARGIN and cons <= CONSERVED
    assert np.abs(r["win_a"] - r["win_b"]).max() > 0.01


# ---- 6. refusals and side effects -------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    uni = np.full((761, 5), 0.2)
    one = SoccerSimultaneousEnv(width=5, height=4, player_b_policy=[0] * 761)
    with pytest.raises(AssertionError, match="two-player"):
        pl.match_outcomes(one, uni, uni, THETA, C)
    with pytest.raises(AssertionError, match="two-player handle"):
        one._batch.match_outcomes(uni, uni, THETA, C)
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=True)
    for n in (0, 1025):
        many = np.full((n, 761, 5), 0.2)
        with pytest.raises(AssertionError, match="must be 1 .. 1024, not %d and 1" % n):
            b.match_outcomes(many, uni, THETA, C)
        with pytest.raises(AssertionError, match="must be 1 .. 1024, not 1 and %d" % n):
            b.match_outcomes(uni, many, THETA, C)
    for ppp in (63, -64):
        with pytest.raises(AssertionError, match="pairs_per_pass must be 0 .* or a positive multiple of 64, not %d" % ppp):
            b.match_outcomes(uni, uni, THETA, C, pairs_per_pass=ppp)
    for c in (1.5, -0.1, float("nan")):
        with pytest.raises(AssertionError, match="continue_prob"):
            b.match_outcomes(uni, uni, THETA, c)
    with pytest.raises(AssertionError, match="max_sweeps"):
        b.match_outcomes(uni, uni, THETA, C, max_sweeps=0)
    with pytest.raises(AssertionError, match="theta"):
        b.match_outcomes(uni, uni, -1.0, C)
    for bad, msg in ((-0.1, "negative or not a number"), (0.1, "does not sum to 1")):
        pol = np.full((3, 761, 5), 0.2)
        pol[1, 37, 2] = bad                                            # (0.1: the row sums to 0.9)
        with pytest.raises(AssertionError, match=r"soccer_match_outcomes: pi_a\[1\]\[37\].*" + msg):
            b.match_outcomes(pol, np.full((2, 761, 5), 0.2), THETA, C)
        with pytest.raises(AssertionError, match=r"soccer_match_outcomes: pi_b\[1\]\[37\].*" + msg):
            b.match_outcomes(np.full((2, 761, 5), 0.2), pol, THETA, C)
    # row 0 is not read
    pol = np.full((2, 761, 5), 0.2)
    want = b.match_outcomes(pol, pol, THETA, C, values=True)
    pol[:, 0] = np.nan
    same_result(b.match_outcomes(pol, pol, THETA, C, values=True), want, "a matrix with another row 0")
    b.close()


def test_capture_no_ticks_and_the_lanes_are_left_alone():
    A, B = sets(5, 4, 0.0, 3, 5)
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=True)
    b.reset()
    n = 64
    a = b.alloc(n, np.int8).fill(0); c = b.alloc(n, np.int8).fill(1)
    obs = b.alloc(n, np.uint16); rew = b.alloc(n, np.int8); term = b.alloc(n, np.uint8); trunc = b.alloc(n, np.uint8)
    b.graph_begin()
    b.step_plain(a, c, obs, rew, term, trunc)
    with pytest.raises(RuntimeError, match="graph capture"):
        b.match_outcomes(A, B, THETA, C)
    b.graph_destroy(b.graph_end())
    b.close()
    # a completed, a capped and a refused call consume no tick and leave the lanes alone: the same rollout with and without
    outs = []
    for solve in (False, True):
        env = VectorSoccerEnv(1024, slip_prob=0.2, seed=3)
        env.reset()
        if solve:
            tick = env.batch.tick
            A2, B2 = sets(5, 4, 0.2, 3, 5)
            r = env.match_outcomes(A2, B2, THETA, C)
            same_result(pl.match_outcomes(env, A2, B2, THETA, C), r, "planners.match_outcomes against the environment's")
            with pytest.raises(RuntimeError, match="had not converged"):
                env.match_outcomes(A2, B2, THETA, C, max_sweeps=3)
            with pytest.raises(AssertionError, match="pairs_per_pass"):
                env.match_outcomes(A2, B2, THETA, C, pairs_per_pass=65)
            assert env.batch.tick == tick
        O, R, TE, TR, _ = env.rollout(20, sample_actions=True)
        outs.append((O["player_a"].copy(), R["player_a"].copy(), TE["player_a"].copy(), TR["player_a"].copy()))
        env.close()
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x, y)


# ---- 7. populations ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["q", "wolf", "minimax_q", "om"])
def test_a_population_s_match_outcomes_is_the_batch_s_on_what_read_returns(kind):
    n = 67
    make = {"q": lambda b, g: b.q_population(g), "wolf": lambda b, g: b.wolf_population(g),
            "minimax_q": lambda b, g: b.minimax_q_population(g), "om": lambda b, g: b.om_population(g)}[kind]
    b = SoccerBatch(n, 5, 4, 0.2, seed=7, autoreset=True)
    pop = make(b, C)
    b.reset(); pop.run(40)
    r = pop.read()
    got = pop.match_outcomes()
    assert got["win_a"].shape == (n, n) and "values" not in got
    same_result(got, b.match_outcomes(r["pi_a"], r["pi_b"], THETA, C), "the population's matrix")
    part = pop.match_outcomes(first=1, count=3, continue_prob=0.5, theta=1e-8)
    same_result(part, b.match_outcomes(r["pi_a"][1:4], r["pi_b"][1:4], 1e-8, 0.5), "members 1 .. 3 at another continuation probability")
    if kind == "wolf":
        same_result(pop.match_outcomes(which="avg"), b.match_outcomes(r["avg_a"], r["avg_b"], THETA, C), "the average policies' matrix")
    if kind == "om":
        same_result(pop.match_outcomes("model"), b.match_outcomes(r["model_a"], r["model_b"], THETA, C), "the models' matrix")
    pop.close()
    gam = np.full(n, 0.9); gam[2] = 0.8
    mixed = make(b, gam)
    with pytest.raises(ValueError, match="members 0 and 2 have different discounts .* pass continue_prob"):
        mixed.match_outcomes()
    assert mixed.match_outcomes(count=2)["win_a"].shape == (2, 2)               # members 0 and 1 share theirs
    assert mixed.match_outcomes(first=1, count=3, continue_prob=0.9)["length"].shape == (3, 3)
    mixed.close(); b.close()


# ---- 8. a large pitch -------------------------------------------------------------------------------------------------------
def test_a_large_pitch():
    """c = 0.5: no channel moves by more than 0.5^(k-1) in sweep k, so every pair stops within 35 sweeps"""
    w, h, slip, c = 11, 7, 0.2, 0.5
    A, B = policy_set(w, h, slip, 2, 31), policy_set(w, h, slip, 3, 32)
    b = SoccerBatch(1, w, h, slip)
    assert b.nS == 11705
    got = b.match_outcomes(A, B, THETA, c, values=True)
    b.close()
    print("11x7: win_a %s win_b %s length %s sweeps %s" % (np.round(got["win_a"], 6).tolist(), np.round(got["win_b"], 6).tolist(),
                                                            np.round(got["length"], 6).tolist(), got["iterations"].tolist()))
    assert got["iterations"].max() <= 35
    flat = [0, 4, 5]                                                    # 3 of the 6 pairs: the first, one of each row, the last
    want = mon.match_outcomes(oracle_lists(w, h, slip), starts_of(w, h, slip), A, B, c, THETA, pairs=flat)
    for n, f in enumerate(flat):
        for k in KEYS:
            same_bits(got[k][f // 3, f % 3], want[k][n], "%s of pair %d" % (k, f))
