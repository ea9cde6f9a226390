"""Exact policy gradients and gradient play on the device (soccer_policy_gradient, soccer_gradient_play_*): every sampled pair to
the bits and the sweep counts of the numpy restatement (tests/policy_gradient_np.py) on every matrix shape; a whole matrix, so
the weighted sums too, with and without weights and normalisation; rows that span passes; no result depends on how the matrix is
cut into passes, on what the handle's buffers held before or on which outputs are asked for; the sweep cap with solves open in V
only, in D only and in both; the refusals; the learner against the restatement and against rounds of the public call; and a
large pitch."""
import os
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch, SoccerSimultaneousEnv, VectorSoccerEnv
from gym_soccer_littman94_amd import planners as pl

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_gradient_np as pgn  # noqa: E402
from test_gpu_best_response import oracle_lists, same_bits  # noqa: E402
from test_gpu_cross_play import policy_set  # noqa: E402
from test_gpu_match_outcomes import C_OF, NB, PITCHES, SAMPLE, SHAPES, THETA, sets, starts_of  # noqa: E402
from test_gpu_occupancy import in_lists  # noqa: E402  (computed once per pitch for both modules)

pytestmark = pytest.mark.gpu

GAMMA = 0.9
PAIR_KEYS = ("payoff", "q_a", "q_b", "V", "occupancy", "iterations")
SUM_KEYS = ("grad_a", "grad_b", "reach_a", "reach_b")
ALL_KEYS = PAIR_KEYS + SUM_KEYS

_want, _full = {}, {}


def restate(w, h, slip, A, B, gamma, theta=THETA, **kw):
    return pgn.policy_gradient(oracle_lists(w, h, slip), starts_of(w, h, slip), A, B, gamma, theta, inl=in_lists(w, h, slip), **kw)


def restate_pairs(w, h, slip, A, B, flat, gamma, theta=THETA):
    """the per-pair arrays of the pairs with flat indices i * len(B) + j"""
    flat = np.asarray(flat)
    return pgn.pairs(oracle_lists(w, h, slip), starts_of(w, h, slip), A[flat // len(B)], B[flat % len(B)], gamma, theta,
                     inl=in_lists(w, h, slip))


def restated(w, h, slip):
    """{(i, j): the restatement's per-pair dict} for the pairs of SAMPLE, computed once per pitch"""
    if (w, h, slip) not in _want:
        A, B = sets(w, h, slip)
        r = restate_pairs(w, h, slip, A, B, [i * NB + j for i, j in SAMPLE], C_OF[(w, h, slip)])
        _want[(w, h, slip)] = {ij: {k: r[k][n] for k in PAIR_KEYS} for n, ij in enumerate(SAMPLE)}
    return _want[(w, h, slip)]


def full_7x67(w, h, slip):
    """(A, B, the uncapped 7 x 67 result with everything asked for) on a handle of its own, computed once"""
    if (w, h, slip) not in _full:
        A, B = sets(w, h, slip, 7, 67)
        b = SoccerBatch(1, w, h, slip)
        _full[(w, h, slip)] = (A, B, b.policy_gradient(A, B, THETA, GAMMA, values=True))
        b.close()
    return _full[(w, h, slip)]


def same_result(got, want, what, keys=None):
    if keys is None:
        assert sorted(got) == sorted(want), (sorted(got), sorted(want))
        keys = sorted(want)
    for k in keys:
        same_bits(got[k], want[k], "%s of %s" % (k, what))


def capped(call):
    try:
        return call(), None
    except RuntimeError as e:
        return e.results, str(e)


# ---- 1. every shape against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,slip", PITCHES)
def test_sampled_pairs_of_every_shape_are_the_restatement_s_bits(w, h, slip):
    want, gamma = restated(w, h, slip), C_OF[(w, h, slip)]
    b = SoccerBatch(1, w, h, slip)
    for n_a, n_b in SHAPES:
        A, B = sets(w, h, slip, n_a, n_b)
        got = b.policy_gradient(A, B, THETA, gamma, values=True)
        assert sorted(got) == sorted(ALL_KEYS)
        assert got["payoff"].shape == (n_a, n_b) and got["iterations"].shape == (n_a, n_b, 2) and got["iterations"].dtype == np.int64
        assert got["q_a"].shape == got["q_b"].shape == (n_a, n_b, b.nS, 5) and got["V"].shape == got["occupancy"].shape == (n_a, n_b, b.nS)
        assert got["grad_a"].shape == (n_a, b.nS, 5) and got["grad_b"].shape == (n_b, b.nS, 5)
        assert got["reach_a"].shape == (n_a, b.nS) and got["reach_b"].shape == (n_b, b.nS)
        inside = [(i, j) for i, j in SAMPLE if i < n_a and j < n_b]
        print("%dx%d slip %.1f, %d x %d: %d of %d pairs restated" % (w, h, slip, n_a, n_b, len(inside), n_a * n_b))
        assert (0, 0) in inside and (n_a - 1, n_b - 1) in inside
        for i, j in inside:
            for k in PAIR_KEYS:
                same_bits(got[k][i, j], want[(i, j)][k], "%s of pair (%d, %d) of %d x %d" % (k, i, j, n_a, n_b))
        assert (got["q_a"][:, :, 0] == 0).all() and (got["q_b"][:, :, 0] == 0).all() and (got["grad_a"][:, 0] == 0).all()
        # the weighted sums are the sequential sums of the returned per-pair arrays (7 x 67: every row spans passes of 64)
        sums = pgn.reduce(got["occupancy"], got["q_a"], got["q_b"])
        for k, s in zip(SUM_KEYS, sums):
            same_bits(got[k], s, "%s of %d x %d from its pairs" % (k, n_a, n_b))
    it = got["iterations"]
    print("%dx%d slip %.1f, 7 x 67 at gamma %.1f: V sweeps %d .. %d, D sweeps %d .. %d" % (
        w, h, slip, gamma, it[..., 0].min(), it[..., 0].max(), it[..., 1].min(), it[..., 1].max()))
    assert (it[..., 0] != it[..., 1]).any()
    one = b.policy_gradient(A[2], B[5], THETA, gamma, values=True)      # a single [nS, 5] policy is a batch of one
    same_result(one, {k: got[k][2:3, 5:6] for k in PAIR_KEYS}, "a single pair", keys=PAIR_KEYS)
    same_bits(one["grad_a"], 0.0 + one["occupancy"][0, :, :, None] * one["q_a"][0], "a single pair's grad_a")
    b.close()


# ---- 2. a whole matrix: the weighted sums, the weights, the normalisation ----------------------------------------------------
@pytest.mark.parametrize("slip", [0.0, 0.2])
def test_the_whole_3x5_matrix_with_and_without_weights_and_normalisation(slip):
    w, h = 5, 4
    A, B = sets(w, h, slip, 3, 5)
    base = restate(w, h, slip, A, B, GAMMA)
    b = SoccerBatch(1, w, h, slip)
    w_a, w_b = np.array([0.5, 0.0, 0.3]), np.array([0.1, 0.0, 0.2, 1.0 / 3.0, 7.0])       # a zero, non-dyadic ones, no unit sum
    for wa, wb in ((None, None), (w_a, w_b)):
        for normalize in (False, True):
            want = dict(base)
            want.update(zip(SUM_KEYS, pgn.reduce(base["occupancy"], base["q_a"], base["q_b"], wa, wb, normalize)))
            got = b.policy_gradient(A, B, THETA, GAMMA, w_a=wa, w_b=wb, normalize=normalize, values=True)
            same_result(got, want, "3 x 5 (weights %s, normalize %s)" % (wa is not None, normalize))
            same_result(pl.policy_gradient(b, A, B, THETA, GAMMA, w_a=wa, w_b=wb, normalize=normalize, values=True), got, "planners'")
            assert np.isfinite(got["grad_a"]).all() and np.isfinite(got["grad_b"]).all()
    assert (np.abs(got["grad_a"]) > 0.01).any()
    if slip == 0.0:                                                     # without slip, one-hot policies never reach some states
        assert (got["reach_a"][:, 1:] == 0).any() and (got["grad_a"][got["reach_a"] == 0] == 0).all()
    b.close()


# ---- 3. passes, cached buffers, what is asked for, and the siblings' bits ---------------------------------------------------------
def test_no_result_depends_on_the_passes_on_earlier_calls_or_on_what_is_asked_for():
    w, h, slip = 5, 4, 0.2
    A, B, want = full_7x67(w, h, slip)
    b = SoccerBatch(1, w, h, slip)
    small_first = b.policy_gradient(A[:3], B[:5], THETA, GAMMA, values=True)               # (buffers for 64 pairs, regrown below)
    for ppp in (64, 128, 448, 0):
        same_result(b.policy_gradient(A, B, THETA, GAMMA, values=True, pairs_per_pass=ppp), want, "7 x 67 with pairs_per_pass = %d" % ppp)
    same_result(b.policy_gradient(A[:3], B[:5], THETA, GAMMA, values=True), small_first, "3 x 5 after 7 x 67, against a fresh handle's")
    same_result(small_first, {k: want[k][:3, :5] for k in PAIR_KEYS}, "3 x 5 as a corner of 7 x 67", keys=PAIR_KEYS)
    # after a call that failed: at the cap, and refused
    with pytest.raises(RuntimeError, match="469 of 469 pairs had not converged after max_sweeps = 3"):
        b.policy_gradient(A, B, THETA, GAMMA, max_sweeps=3, pairs_per_pass=128)
    with pytest.raises(AssertionError, match="pairs_per_pass"):
        b.policy_gradient(A, B, THETA, GAMMA, pairs_per_pass=63)
    same_result(b.policy_gradient(A, B, THETA, GAMMA, values=True, pairs_per_pass=64), want, "7 x 67 after two failed calls")
    # without the values
    got = b.policy_gradient(A, B, THETA, GAMMA, pairs_per_pass=64)
    assert sorted(got) == sorted(("payoff", "iterations") + SUM_KEYS)
    same_result(got, want, "7 x 67 without values", keys=sorted(got))
    # the C call with every output NULL but one
    nS = b.nS
    shapes = {"payoff": (7, 67), "grad_a": (7, nS, 5), "grad_b": (67, nS, 5), "reach_a": (7, nS), "reach_b": (67, nS),
              "q_a": (7, 67, nS, 5), "q_b": (7, 67, nS, 5), "V": (7, 67, nS), "occupancy": (7, 67, nS), "iterations": (7, 67, 2)}
    order = list(shapes)
    for key in ("payoff", "grad_b", "reach_a", "q_b", "occupancy", "iterations"):
        out = np.zeros(shapes[key], np.int32 if key == "iterations" else np.float64)
        ptr = [out.ctypes.data if k == key else None for k in order]
        b._check(b.lib.soccer_policy_gradient(b.h, 7, A.ctypes.data, 67, B.ctypes.data, THETA, GAMMA, 1000000, 128, None, None, 0, *ptr))
        same_bits(out.astype(want[key].dtype), want[key], key + " alone")
    # the siblings' bits on the same handle
    payoff, it, V = b.cross_play(A, B, THETA, GAMMA, values=True)
    occ = b.occupancy(A, B, THETA, GAMMA, values=True)
    same_bits(want["payoff"], payoff, "payoff against cross_play's"); same_bits(want["V"], V, "V against cross_play's")
    same_bits(want["occupancy"], occ["occupancy"], "occupancy against occupancy's")
    same_bits(want["iterations"], np.stack([it, occ["iterations"]], -1), "iterations against the siblings'")
    same_result(b.policy_gradient(A, B, THETA, GAMMA, values=True), want, "7 x 67 after the siblings")
    b.close()


# ---- 4. the sweep cap -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta", [THETA, 1e-3])
def test_the_sweep_cap_marks_the_open_solves_and_keeps_their_last_iterates(theta):
    w, h, slip = 5, 4, 0.2
    A, B = sets(w, h, slip, 3, 5)
    free = restate(w, h, slip, A, B, GAMMA, theta, max_sweeps=34)["iterations"]           # a solve still open after 34 is open at every cap
    print("theta %g: sweeps (V, D) of the 3 x 5 pairs, 34 for more\n%s" % (theta, free.reshape(15, 2).T))
    b = SoccerBatch(1, w, h, slip)
    w_b = np.array([0.1, 0.0, 0.2, 1.0 / 3.0, 7.0])
    seen = set()
    for cap in (1, 16, 17, 33):
        want = restate(w, h, slip, A, B, GAMMA, theta, w_b=w_b, normalize=True, max_sweeps=cap)
        late = free > cap
        open_pairs = late.any(-1)
        seen |= {(bool(v), bool(d)) for v, d in late.reshape(-1, 2)}
        got, msg = capped(lambda: b.policy_gradient(A, B, theta, GAMMA, w_b=w_b, normalize=True, values=True, max_sweeps=cap))
        if open_pairs.any():
            assert msg is not None and "%d of 15 pairs had not converged after max_sweeps = %d" % (open_pairs.sum(), cap) in msg, msg
        else:
            assert msg is None
        same_bits(got["iterations"], np.where(late, cap, free), "iterations at a cap of %d" % cap)
        same_result(got, want, "the 3 x 5 matrix at a cap of %d" % cap)
    if theta == THETA:
        assert (free > 33).all()
    else:
        print("theta %g: (V open, D open) combinations met at the caps: %s" % (theta, sorted(seen)))
        assert seen == {(False, False), (True, False), (False, True), (True, True)}      # open in V only, in D only, in both
    b.close()


# ---- 5. refusals and side effects -------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_cost_no_tick():
    uni = np.full((761, 5), 0.2)
    one = SoccerSimultaneousEnv(width=5, height=4, player_b_policy=[0] * 761)
    with pytest.raises(AssertionError, match="two-player"):
        pl.policy_gradient(one, uni, uni, THETA, GAMMA)
    with pytest.raises(AssertionError, match="two-player handle"):
        one._batch.policy_gradient(uni, uni, THETA, GAMMA)
    with pytest.raises(AssertionError, match="two-player handle"):
        one._batch.gradient_play()
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=True)
    b.reset()
    tick = b.tick
    for n in (0, 1025):
        many = np.full((n, 761, 5), 0.2)
        with pytest.raises(AssertionError, match="must be 1 .. 1024, not %d and 1" % n):
            b.policy_gradient(many, uni, THETA, GAMMA)
        with pytest.raises(AssertionError, match="must be 1 .. 1024, not 1 and %d" % n):
            b.policy_gradient(uni, many, THETA, GAMMA)
        with pytest.raises(AssertionError, match="must be 1 .. 1024, not %d and 1" % n):
            b.gradient_play(n_a=n)
    two = np.full((2, 761, 5), 0.2)
    for bad, msg in (([0.5, -0.1], r"w_b\[1\] is negative or not finite"), ([float("nan"), 1.0], r"w_b\[0\] is negative or not finite"),
                     ([1.0, float("inf")], r"w_b\[1\] is negative or not finite"), ([0.0, 0.0], "w_b is all zero")):
        with pytest.raises(AssertionError, match="soccer_policy_gradient: " + msg):
            b.policy_gradient(uni, two, THETA, GAMMA, w_b=bad)
        with pytest.raises(AssertionError, match="soccer_policy_gradient: " + msg.replace("w_b", "w_a")):
            b.policy_gradient(two, uni, THETA, GAMMA, w_a=bad)
    with pytest.raises(AssertionError, match="one weight per policy"):
        b.policy_gradient(uni, two, THETA, GAMMA, w_b=[1.0])
    for ppp in (65, -64):
        with pytest.raises(AssertionError, match="pairs_per_pass must be 0 .* or a positive multiple of 64, not %d" % ppp):
            b.policy_gradient(uni, uni, THETA, GAMMA, pairs_per_pass=ppp)
    for g in (1.5, -0.1, float("nan")):
        with pytest.raises(AssertionError, match="discount_factor"):
            b.policy_gradient(uni, uni, THETA, g)
    with pytest.raises(AssertionError, match="max_sweeps"):
        b.policy_gradient(uni, uni, THETA, GAMMA, max_sweeps=0)
    with pytest.raises(AssertionError, match="theta"):
        b.policy_gradient(uni, uni, -1.0, GAMMA)
    pol = np.full((3, 761, 5), 0.2)
    pol[1, 37, 2] = 0.1
    with pytest.raises(AssertionError, match=r"soccer_policy_gradient: pi_a\[1\]\[37\].*does not sum to 1"):
        b.policy_gradient(pol, uni, THETA, GAMMA)
    with pytest.raises(AssertionError, match=r"soccer_gradient_play_create: pi_b\[1\]\[37\].*does not sum to 1"):
        b.gradient_play(n_b=3, pi_b=pol)
    for kw, msg in (({"eta_a": -1.0}, "eta_a and eta_b"), ({"eta_b": float("inf")}, "eta_a and eta_b"), ({"optimism": 1.5}, "optimism")):
        with pytest.raises(AssertionError, match=msg):
            b.gradient_play(**kw)
    # during a capture
    n = 64
    a = b.alloc(n, np.int8).fill(0); c = b.alloc(n, np.int8).fill(1)
    obs = b.alloc(n, np.uint16); rew = b.alloc(n, np.int8); term = b.alloc(n, np.uint8); trunc = b.alloc(n, np.uint8)
    g = b.gradient_play(theta=1e-3)
    b.graph_begin()
    b.step_plain(a, c, obs, rew, term, trunc)
    with pytest.raises(RuntimeError, match="soccer_policy_gradient during graph capture"):
        b.policy_gradient(uni, uni, THETA, GAMMA)
    with pytest.raises(RuntimeError, match="soccer_gradient_play_run during graph capture"):
        g.run(1)
    with pytest.raises(RuntimeError, match="graph capture"):
        b.gradient_play()
    b.graph_destroy(b.graph_end())
    # a completed call, a capped one and a learner's steps consume no tick either
    b.policy_gradient(uni, uni, 1e-3, GAMMA)
    with pytest.raises(RuntimeError, match="had not converged"):
        b.policy_gradient(uni, uni, THETA, GAMMA, max_sweeps=2)
    g.run(2)
    assert g.read()["steps"] == 2 and b.tick == tick
    other = SoccerBatch(1, 5, 4, 0.0)
    with pytest.raises(AssertionError, match="not a gradient-play learner of this handle"):
        other._check(other.lib.soccer_gradient_play_run(other.h, g.q, 1, None))
    other.close()
    g.close(); b.close()


def test_the_environment_s_calls_leave_the_lanes_alone():
    outs = []
    for solve in (False, True):
        env = VectorSoccerEnv(1024, slip_prob=0.2, seed=3)
        env.reset()
        if solve:
            tick = env.batch.tick
            A2, B2 = sets(5, 4, 0.2, 2, 3)
            r = env.policy_gradient(A2, B2, 1e-6, 0.5, values=True)
            same_result(pl.policy_gradient(env, A2, B2, 1e-6, 0.5, values=True), r, "planners.policy_gradient against the environment's")
            g = env.gradient_play(n_a=2, n_b=3, discount_factor=0.5, theta=1e-6, pi_a=A2, pi_b=B2)
            tr = g.run(2, trace=True)
            same_bits(tr[0], r["payoff"], "the first step's payoff matrix")
            out = pl.gradient_play(env, 2, 0.5, n_a=2, n_b=3, theta=1e-6, pi_a=A2, pi_b=B2)
            same_bits(out["trace"], tr, "planners.gradient_play's trace"); same_bits(out["pi_a"], g.read()["pi_a"], "... and its policies")
            g.close()
            assert env.batch.tick == tick
        O, R, TE, TR, _ = env.rollout(20, sample_actions=True)
        outs.append((O["player_a"].copy(), R["player_a"].copy(), TE["player_a"].copy(), TR["player_a"].copy()))
        env.close()
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x, y)


# ---- 6. gradient play ---------------------------------------------------------------------------------------------------------
def same_state(r, x, y, prev_a, prev_b, steps, what):
    same_bits(r["pi_a"], x, "pi_a " + what); same_bits(r["pi_b"], y, "pi_b " + what)
    same_bits(r["prev_a"], prev_a, "prev_a " + what); same_bits(r["prev_b"], prev_b, "prev_b " + what)
    assert r["steps"] == steps


@pytest.mark.parametrize("slip,n_a,n_b,steps,kw", [
    (0.0, 2, 3, 3, dict(eta_a=1.0, eta_b=0.5, optimism=0.5, normalize=True, w_a=[0.25, 0.75], w_b=[0.5, 0.2, 0.3])),
    (0.2, 1, 1, 2, dict(eta_a=4.0, eta_b=8.0, optimism=0.0, normalize=False, w_a=None, w_b=None)),
    (0.0, 1, 2, 2, dict(eta_a=1.0, eta_b=0.0, optimism=1.0, normalize=True, w_a=None, w_b=[0.25, 0.75]))])     # a fixed league
def test_gradient_play_is_the_restatement_s(slip, n_a, n_b, steps, kw):
    w, h = 5, 4
    A, B = policy_set(w, h, slip, 5, 31)[3:3 + n_a], policy_set(w, h, slip, 5, 32)[2:2 + n_b]    # Dirichlet and one-hot rows among them
    x, y, prev_a, prev_b, trace = pgn.gradient_play(oracle_lists(w, h, slip), starts_of(w, h, slip), A, B, steps, GAMMA, THETA,
                                                    inl=in_lists(w, h, slip), **kw)
    b = SoccerBatch(1, w, h, slip)
    g = b.gradient_play(n_a=n_a, n_b=n_b, discount_factor=GAMMA, eta_a=kw["eta_a"], eta_b=kw["eta_b"], optimism=kw["optimism"],
                        normalize=kw["normalize"], theta=THETA, pi_a=A, pi_b=B)
    g.weights(kw["w_a"], kw["w_b"])
    got = g.run(steps, trace=True)
    same_bits(got, trace, "the trace")
    r = g.read()
    same_state(r, x, y, prev_a, prev_b, steps, "after %d steps" % steps)
    same_bits(r["payoff"], trace[-1], "the last step's payoff")
    assert (bits_differ(r["pi_a"][:, 1:], A[:, 1:]) and (r["pi_a"] >= 0).all() and np.abs(r["pi_a"][:, 1:].sum(2) - 1).max() < 1e-14)
    same_bits(r["pi_a"][:, 0], A[:, 0], "row 0 is never touched")
    if kw["eta_b"] == 0.0:                                              # held fixed to the bit, where a projection would move it
        same_bits(r["pi_b"], B, "a side whose step is 0")
        assert bits_differ(pgn.project(B[:, 1:]), B[:, 1:]) and (r["prev_b"] != 0).any()
    b.policy_gradient(r["pi_a"], r["pi_b"], 1e-3, GAMMA)                # projected rows pass the row check
    g.close(); b.close()


def bits_differ(a, b):
    return (np.ascontiguousarray(a).view(np.int64) != np.ascontiguousarray(b).view(np.int64)).any()


def test_gradient_play_is_rounds_of_the_public_call_plus_the_numpy_update():
    w, h, slip = 5, 4, 0.2
    A, B = sets(w, h, slip, 64, 2)
    kw = dict(n_a=64, n_b=2, discount_factor=0.5, eta_a=2.0, eta_b=1.0, optimism=1.0, normalize=True, theta=1e-8, pi_a=A, pi_b=B)
    b = SoccerBatch(1, w, h, slip)
    g = b.gradient_play(**kw)
    r0 = g.read()
    same_bits(r0["pi_a"], A, "pi_a as created"); same_bits(r0["w_a"], np.full(64, 1.0 / 64), "uniform weights")
    assert r0["steps"] == 0 and (r0["prev_a"] == 0).all()
    # five rounds by hand; the weights change after the third
    w_a2, w_b2 = np.linspace(0.0, 1.0, 64), np.array([0.9, 0.1])
    x, y, prev_a, prev_b, trace, states = A, B, np.zeros(A.shape), np.zeros(B.shape), [], []
    for t in range(5):
        wa, wb = (None, None) if t < 3 else (w_a2, w_b2)
        r = b.policy_gradient(x, y, 1e-8, 0.5, w_a=wa, w_b=wb, normalize=True)
        trace.append(r["payoff"])
        x, y, prev_a, prev_b = pgn.step(x, y, r["grad_a"], r["grad_b"], prev_a, prev_b, t == 0, 2.0, 1.0, 1.0)
        states.append((x, y, prev_a, prev_b))
    got = [g.run(3, trace=True)]
    same_state(g.read(), *states[2], 3, "after three steps")
    saved = g.read()
    # a capped step leaves the state untouched
    g2 = b.gradient_play(**dict(kw, max_sweeps=2))
    g2.load(**saved)
    with pytest.raises(RuntimeError, match="soccer_gradient_play_run: 128 of 128 pairs had not converged") as e:
        g2.run(2, trace=True)
    assert (e.value.results == 0).all()
    same_result(g2.read(), saved, "the state after a capped step")
    g2.close()
    # set_weights takes effect at the next step
    g.weights(w_a2, w_b2)
    got.append(g.run(2, trace=True))
    same_bits(np.concatenate(got), np.stack(trace), "the trace of 3 + 2 steps")
    r = g.read()
    same_state(r, *states[4], 5, "after five steps")
    same_bits(r["w_a"], w_a2, "w_a"); same_bits(r["w_b"], w_b2, "w_b"); same_bits(r["payoff"], trace[4], "the last payoff")
    # load(read()) onto a fresh learner continues identically
    fresh = b.gradient_play(**dict(kw, pi_a=None, pi_b=None))
    assert (fresh.read()["pi_b"] == 0.2).all()
    fresh.load(**saved).weights(w_a2, w_b2)
    same_bits(fresh.run(2, trace=True), got[1], "the fresh learner's trace")
    same_result(fresh.read(), r, "the fresh learner's state")
    # the derived calls are the public ones on what read() returns
    same_bits(g.cross_play()["payoff"], b.cross_play(r["pi_a"], r["pi_b"], 1e-8, 0.5)[0], "cross_play of the current sets")
    fresh.close(); g.close(); b.close()


def test_self_play_from_the_uniform_pair_closes_the_gap():
    b = SoccerBatch(1, 5, 4, 0.0)
    starts = starts_of(5, 4, 0.0)
    g = b.gradient_play(discount_factor=GAMMA, eta_a=1.0, eta_b=1.0, normalize=True, theta=1e-10)
    before = g.exploitability()["gap"][0, starts].mean()
    g.run(10)
    after = g.exploitability()["gap"][0, starts].mean()
    print("kick-off exploitability of the uniform pair %.4f, after 10 normalised steps %.4f" % (before, after))
    assert after < 0.5 * before
    m = g.meta_game()
    assert m["payoff"].shape == (1, 1) and m["lo"] <= m["hi"]
    g.close(); b.close()


# ---- 7. a large pitch -------------------------------------------------------------------------------------------------------
def test_a_large_pitch():
    w, h, slip, gamma = 11, 7, 0.2, 0.5
    A, B = policy_set(w, h, slip, 2, 31), policy_set(w, h, slip, 3, 32)
    b = SoccerBatch(1, w, h, slip)
    assert b.nS == 11705
    got = b.policy_gradient(A, B, THETA, gamma, values=True)
    b.close()
    print("11x7: payoff %s sweeps %s" % (np.round(got["payoff"], 6).tolist(), got["iterations"].tolist()))
    assert got["iterations"].max() <= 36
    flat = [0, 4, 5]                                                    # 3 of the 6 pairs: the first, one of each row, the last
    want = restate_pairs(w, h, slip, A, B, flat, gamma)
    for n, f in enumerate(flat):
        for k in PAIR_KEYS:
            same_bits(got[k][f // 3, f % 3], want[k][n], "%s of pair %d" % (k, f))
    for k, s in zip(SUM_KEYS, pgn.reduce(got["occupancy"], got["q_a"], got["q_b"])):
        same_bits(got[k], s, k + " from its pairs")
