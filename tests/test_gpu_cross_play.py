"""Cross-play on the device (soccer_cross_play): every pair of the matrix to the bits and the sweep count that
soccer_evaluate_policies gives that pair, and to those of the numpy restatement (tests/cross_play_np.py); no result depends on
how the matrix is cut into passes or on what the handle's buffers held before; the sweep cap; a large pitch; the refusals; the
three populations; and every value between the worst cases of its two policies."""
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
from test_gpu_best_response import minimax, oracle_lists, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

GAMMA, THETA = 0.9, 1e-10
PITCHES = [(5, 4, 0.0), (5, 4, 0.2), (7, 5, 0.3)]
SHAPES = [(1, 1), (3, 5), (64, 2), (7, 67)]
MARGIN = 2 * GAMMA * THETA / (1 - GAMMA)           # two fixed points of one modulus, each stopped at theta

_sets, _full = {}, {}


def policy_set(w, h, slip, n, seed):
    """n policies drawn like test_gpu_best_response.policies: uniform, the two minimax strategies, Dirichlet rows of two
    concentrations and one-hot rows in turn, every random one a fresh draw — easy and hard ones side by side"""
    if (w, h, slip, n, seed) not in _sets:
        pa, pb, _ = minimax(w, h, slip)
        nS = pa.shape[0]
        rng = np.random.default_rng(seed)
        kinds = [lambda: np.full((nS, 5), 0.2), lambda: pa, lambda: pb, lambda: rng.dirichlet(np.ones(5), nS),
                 lambda: rng.dirichlet(np.full(5, 0.2), nS), lambda: brn.onehot(rng.integers(0, 5, nS))]
        _sets[(w, h, slip, n, seed)] = np.stack([kinds[(k + seed) % 6]() for k in range(n)])
    return _sets[(w, h, slip, n, seed)]


def sets(w, h, slip, n_a, n_b):
    return policy_set(w, h, slip, n_a, 31), policy_set(w, h, slip, n_b, 32)


def pairwise(b, A, B, max_sweeps=1000000, theta=THETA, gamma=GAMMA):
    """the same matrix through evaluate_policies, 256 pairs a call: (payoff, iterations, V)"""
    na, nb = len(A), len(B)
    ii, jj = np.divmod(np.arange(na * nb), nb)
    V = np.zeros((na * nb, b.nS)); it = np.zeros(na * nb, np.int64)
    for c in range(0, na * nb, 256):
        s = slice(c, c + 256)
        try:
            V[s], it[s] = b.evaluate_policies(A[ii[s]], B[jj[s]], theta, gamma, max_sweeps=max_sweeps)
        except RuntimeError as e:
            V[s], it[s] = e.results
    starts = kickoff_states(b)
    return cpn.kickoff(V, starts).reshape(na, nb), it.reshape(na, nb), V.reshape(na, nb, b.nS)


def kickoff_states(b):
    """the handle's initial states as observation indices, in ISD order"""
    lut, _, isd = b.tables()
    W = b.internal_width
    H = int(round((b.lut_len // 2) ** 0.5)) // W              # the table has (H * W) ** 2 * 2 entries
    return [int(lut[((((int(s[0]) * W + int(s[1])) * H + int(s[2])) * W + int(s[3])) << 1) | int(s[4])]) for s in isd]


def full_7x67(w, h, slip):
    """(A, B, the uncapped 7 x 67 result with values) on a handle of its own, computed once"""
    if (w, h, slip) not in _full:
        A, B = sets(w, h, slip, 7, 67)
        b = SoccerBatch(1, w, h, slip)
        _full[(w, h, slip)] = (A, B, b.cross_play(A, B, THETA, GAMMA, values=True))
        b.close()
    return _full[(w, h, slip)]


def same_result(got, want, what):
    for name, x, y in zip(("payoff", "iterations", "V"), got, want):
        same_bits(x, y, "%s of %s" % (name, what))


# ---- 1. pair by pair against evaluate_policies ----------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,slip", PITCHES)
def test_every_pair_is_evaluate_policies_on_that_pair(w, h, slip):
    b = SoccerBatch(1, w, h, slip)
    assert kickoff_states(b) == cpn.isd_obs(Oracle(w, h, slip, n=1, seed=0))
    for n_a, n_b in SHAPES:
        A, B = sets(w, h, slip, n_a, n_b)
        got = b.cross_play(A, B, THETA, GAMMA, values=True)
        assert got[0].shape == got[1].shape == (n_a, n_b) and got[2].shape == (n_a, n_b, b.nS) and got[1].dtype == np.int64
        same_result(got, pairwise(b, A, B), "%d x %d" % (n_a, n_b))
        assert (got[2][:, :, 0] == 0).all()
        two = b.cross_play(A, B, THETA, GAMMA)
        assert len(two) == 2
        same_result(two, got[:2], "%d x %d without values" % (n_a, n_b))
    # per-lane stopping: within one wave of 64 pairs the sweep counts are more than a full host batch of 16 apart
    it = got[1].reshape(-1)
    spread = [int(it[c:c + 64].max() - it[c:c + 64].min()) for c in range(0, it.size, 64)]
    print("%dx%d slip %.1f, 7 x 67: sweeps %d .. %d, spread per wave of 64 pairs %s" % (w, h, slip, it.min(), it.max(), spread))
    assert len(spread) == 8 and max(spread) > 16
    # a single [nS, 5] policy is a batch of one
    one = b.cross_play(A[2], B[5], THETA, GAMMA, values=True)
    assert one[0].shape == (1, 1)
    same_result(one, [x[2:3, 5:6] for x in got], "a single pair")
    b.close()


# ---- 2. against the numpy restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,slip", PITCHES)
def test_bit_identical_to_the_numpy_restatement(w, h, slip):
    A, B = sets(w, h, slip, 7, 67)
    A, B = A[[0, 3, 5]], B[[1, 2, 4]]
    b = SoccerBatch(1, w, h, slip)
    got = b.cross_play(A, B, THETA, GAMMA, values=True)
    want = cpn.cross_play(oracle_lists(w, h, slip), cpn.isd_obs(Oracle(w, h, slip, n=1, seed=0)), A, B, GAMMA, THETA)
    print("%dx%d slip %.1f: payoff\n%s\nsweeps %s" % (w, h, slip, np.round(got[0], 6), got[1].tolist()))
    same_result(got, want, "the 3 x 3 matrix")
    r = pl.cross_play(VectorSoccerEnv(4, w, h, slip), A, B, THETA, GAMMA)
    same_bits(r["payoff"], want[0], "planners.cross_play's payoff"); same_bits(r["iterations"], want[1], "its iterations")
    same_bits(r["row_min"], want[0].min(1), "row_min"); same_bits(r["col_max"], want[0].max(0), "col_max")
    assert r["bounds"] == (want[0].min(1).max(), want[0].max(0).min()) and r["bounds"][0] <= r["bounds"][1]
    assert sorted(r) == ["bounds", "col_max", "iterations", "payoff", "row_min"]
    b.close()


# ---- 3. passes and cached buffers -------------------------------------------------------------------------------------------
def test_no_result_depends_on_the_passes_the_buffers_or_the_layout(monkeypatch):
    w, h, slip = 5, 4, 0.2
    A, B, want = full_7x67(w, h, slip)
    b = SoccerBatch(1, w, h, slip)
    small_first = b.cross_play(A[:3], B[:5], THETA, GAMMA, values=True)        # (buffers for 64 pairs, regrown below)
    for ppp in (64, 128, 0, 448, 1024):
        same_result(b.cross_play(A, B, THETA, GAMMA, pairs_per_pass=ppp, values=True), want, "7 x 67 with pairs_per_pass = %d" % ppp)
    same_result(b.cross_play(A[:3], B[:5], THETA, GAMMA, values=True), small_first, "3 x 5 after 7 x 67, against a fresh handle's")
    same_result(small_first, [x[:3, :5] for x in want], "3 x 5 as a corner of 7 x 67")
    same_result(b.cross_play(A, B, THETA, GAMMA, pairs_per_pass=64), want[:2], "7 x 67 in passes of 64 without values")
    b.close()
    monkeypatch.setenv("SOCCER_STATE_LAYOUT", "wide")
    b = SoccerBatch(64, w, h, slip, seed=1, autoreset=True)
    monkeypatch.delenv("SOCCER_STATE_LAYOUT")
    assert b.lib.soccer_state_streams(b.h) == 6
    same_result(b.cross_play(A, B, THETA, GAMMA, values=True), want, "7 x 67 on a handle with the wide layout")
    b.close()


# ---- 4. the sweep cap -------------------------------------------------------------------------------------------------------
def test_the_sweep_cap_leaves_exactly_the_late_pairs_open():
    w, h, slip = 5, 4, 0.2
    A, B, want = full_7x67(w, h, slip)
    ks = want[1]
    median = int(np.median(ks))
    # the median, 1, one that is no multiple of the 16 sweeps between two synchronisations, and one that is
    caps = [median, 1, median + (1 if (median + 1) % 16 else 2), (median // 16) * 16]
    assert caps[2] % 16 and caps[3] % 16 == 0 and caps[3] >= 16
    b = SoccerBatch(1, w, h, slip)
    for cap in caps:
        with pytest.raises(RuntimeError, match="had not converged after max_sweeps = %d" % cap) as e:
            b.cross_play(A, B, THETA, GAMMA, max_sweeps=cap, values=True)
        got = e.value.results
        late = ks > cap
        print("cap %d: %d of %d pairs open" % (cap, late.sum(), late.size))
        assert late.any() and ((~late).any() or cap == 1)
        same_bits(got[1], np.where(late, cap, ks), "iterations at a cap of %d" % cap)
        for name, x, y in zip(("payoff", "iterations", "V"), got, want):
            same_bits(x[~late], y[~late], "%s of the pairs that converged within %d sweeps" % (name, cap))
        # the open pairs hold their last iterate: evaluate_policies stopped at the same sweep
        ref = pairwise(b, A, B, max_sweeps=cap)
        same_result(got, ref, "the matrix at a cap of %d" % cap)
        assert str(late.sum()) + " of 469 pairs" in str(e.value)
    # the capped calls left nothing behind
    same_result(b.cross_play(A, B, THETA, GAMMA, values=True), want, "7 x 67 after the capped calls")
    b.close()


# ---- 5. a large pitch -------------------------------------------------------------------------------------------------------
def test_a_large_pitch():
    w, h, slip = 11, 7, 0.2
    A, B = sets(w, h, slip, 2, 3)
    b = SoccerBatch(1, w, h, slip)
    assert b.nS == 11705
    got = b.cross_play(A, B, THETA, GAMMA, values=True)
    print("11x7: payoff %s sweeps %s" % (np.round(got[0], 6).tolist(), got[1].tolist()))
    same_result(got, pairwise(b, A, B), "2 x 3 on 11x7")
    b.close()


# ---- 6. refusals and side effects -------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    uni = np.full((761, 5), 0.2)
    one = SoccerSimultaneousEnv(width=5, height=4, player_b_policy=[0] * 761)
    with pytest.raises(AssertionError, match="two-player"):
        pl.cross_play(one, uni, uni, THETA, GAMMA)
    with pytest.raises(AssertionError, match="two-player handle"):
        one._batch.cross_play(uni, uni, THETA, GAMMA)
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=True)
    for n in (0, 1025):
        many = np.full((n, 761, 5), 0.2)
        with pytest.raises(AssertionError, match="must be 1 .. 1024, not %d and 1" % n):
            b.cross_play(many, uni, THETA, GAMMA)
        with pytest.raises(AssertionError, match="must be 1 .. 1024, not 1 and %d" % n):
            b.cross_play(uni, many, THETA, GAMMA)
    for ppp in (65, -64, 1):
        with pytest.raises(AssertionError, match="pairs_per_pass must be 0 .* or a positive multiple of 64, not %d" % ppp):
            b.cross_play(uni, uni, THETA, GAMMA, pairs_per_pass=ppp)
    for gamma in (1.5, -0.1, float("nan")):
        with pytest.raises(AssertionError, match="discount_factor"):
            b.cross_play(uni, uni, THETA, gamma)
    with pytest.raises(AssertionError, match="max_sweeps"):
        b.cross_play(uni, uni, THETA, GAMMA, max_sweeps=0)
    with pytest.raises(AssertionError, match="theta"):
        b.cross_play(uni, uni, -1.0, GAMMA)
    with pytest.raises(AssertionError, match="n_states"):
        b.cross_play(np.full((760, 5), 0.2), uni, THETA, GAMMA)
    for bad, msg in ((-0.1, "negative or not a number"), (float("nan"), "negative or not a number"), (0.1, "does not sum to 1")):
        pol = np.full((3, 761, 5), 0.2)
        pol[1, 37, 2] = bad                                            # (0.1: the row sums to 0.9)
        with pytest.raises(AssertionError, match=r"pi_a\[1\]\[37\].*" + msg):
            b.cross_play(pol, np.full((2, 761, 5), 0.2), THETA, GAMMA)
        with pytest.raises(AssertionError, match=r"pi_b\[1\]\[37\].*" + msg):
            b.cross_play(np.full((2, 761, 5), 0.2), pol, THETA, GAMMA)
    # row 0 is not read
    pol = np.full((2, 761, 5), 0.2)
    want = b.cross_play(pol, pol, THETA, GAMMA, values=True)
    pol[:, 0] = np.nan
    same_result(b.cross_play(pol, pol, THETA, GAMMA, values=True), want, "a matrix with another row 0")
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
        b.cross_play(A, B, THETA, GAMMA)
    b.graph_destroy(b.graph_end())
    b.close()
    # a completed, a capped and a refused call consume no tick and leave the lanes alone: the same rollout with and without
    outs = []
    for solve in (False, True):
        env = VectorSoccerEnv(4096, slip_prob=0.2, seed=3)
        env.reset()
        if solve:
            tick = env.batch.tick
            A2, B2 = sets(5, 4, 0.2, 3, 5)
            env.cross_play(A2, B2, THETA, GAMMA)
            with pytest.raises(RuntimeError, match="had not converged"):
                env.cross_play(A2, B2, THETA, GAMMA, max_sweeps=3)
            with pytest.raises(AssertionError, match="pairs_per_pass"):
                env.cross_play(A2, B2, THETA, GAMMA, pairs_per_pass=65)
            assert env.batch.tick == tick
        O, R, TE, TR, _ = env.rollout(50, sample_actions=True)
        outs.append((O["player_a"].copy(), R["player_a"].copy(), TE["player_a"].copy(), TR["player_a"].copy()))
        env.close()
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x, y)


# ---- 7. populations ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["q", "wolf", "minimax_q"])
def test_a_population_s_cross_play_is_the_batch_s_on_what_read_returns(kind):
    n = 5
    make = {"q": lambda b, g: b.q_population(g), "wolf": lambda b, g: b.wolf_population(g),
            "minimax_q": lambda b, g: b.minimax_q_population(g)}[kind]
    b = SoccerBatch(n, 5, 4, 0.2, seed=7, autoreset=True)
    pop = make(b, GAMMA)
    b.reset(); pop.run(200)
    r = pop.read()
    got = pop.cross_play()
    assert got[0].shape == got[1].shape == (n, n)
    same_result(got, b.cross_play(r["pi_a"], r["pi_b"], THETA, GAMMA), "the population's matrix")
    part = pop.cross_play(first=1, count=3, discount_factor=0.5, theta=1e-8)
    same_result(part, b.cross_play(r["pi_a"][1:4], r["pi_b"][1:4], 1e-8, 0.5), "members 1 .. 3 at another discount")
    if kind == "wolf":
        same_result(pop.cross_play("avg"), b.cross_play(r["avg_a"], r["avg_b"], THETA, GAMMA), "the average policies' matrix")
    pop.close()
    gam = np.array([0.9, 0.9, 0.8, 0.9, 0.7])
    mixed = make(b, gam)
    with pytest.raises(ValueError, match="members 0 and 2 have different discounts"):
        mixed.cross_play()
    with pytest.raises(ValueError, match="members 1 and 2 have different discounts"):
        mixed.cross_play(first=1)
    assert mixed.cross_play(count=2)[0].shape == (2, 2)                       # members 0 and 1 share theirs
    assert mixed.cross_play(discount_factor=0.9)[0].shape == (n, n)
    mixed.close(); b.close()


# ---- 8. the bracket ---------------------------------------------------------------------------------------------------------
def test_every_value_lies_between_the_worst_cases_of_its_two_policies():
    w, h, slip = 5, 4, 0.2
    A, B = sets(w, h, slip, 6, 6)
    b = SoccerBatch(1, w, h, slip)
    payoff, it, V = b.cross_play(A, B, THETA, GAMMA, values=True)
    v_a = b.best_response(A, 0, THETA, GAMMA)[1]
    v_b = b.best_response(B, 1, THETA, GAMMA)[1]
    lo = (V - v_a[:, None, :]).min(); hi = (V - v_b[None, :, :]).max()
    print("min (V - v_a) %.3g, max (V - v_b) %.3g, margin %.3g" % (lo, hi, MARGIN))
    assert (V >= v_a[:, None, :] - MARGIN).all() and (V <= v_b[None, :, :] + MARGIN).all()
    assert np.abs(payoff).max() > 0.01
    b.close()
