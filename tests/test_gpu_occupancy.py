"""State occupancy on the device (soccer_occupancy): every sampled pair to the bits and the sweep count of the numpy restatement
(tests/occupancy_np.py) on every matrix shape; per-lane stopping inside a wave; no result depends on how the matrix is cut into
passes, on what the handle's buffers held before or on which outputs are asked for; the finish kernel's sums; the sweep cap; the
game length against match-outcomes' and the reward-weighted sum against cross-play's payoff; the refusals; the populations; and
a large pitch."""
import os
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch, SoccerSimultaneousEnv, VectorSoccerEnv
from gym_soccer_littman94_amd import planners as pl

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occupancy_np as ocn  # noqa: E402
from test_gpu_best_response import oracle_lists, same_bits  # noqa: E402
from test_gpu_cross_play import kickoff_states, policy_set  # noqa: E402
from test_gpu_match_outcomes import C, C_OF, NB, PITCHES, SAMPLE, SHAPES, THETA, noop, sets, starts_of  # noqa: E402
from test_occupancy_np import l1_bound, sup_bound  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("length", "expect", "iterations", "occupancy")
N_F = 3

_want, _full, _inl = {}, {}, {}


def features_of(nS, n_f=N_F):
    """an indicator of every third state, then random weights in [-1, 1); column 0 (the end of the game) is not special"""
    rng = np.random.default_rng(9)
    return np.concatenate([(np.arange(nS) % 3 == 1).astype(np.float64)[None], rng.random((n_f - 1, nS)) * 2 - 1])


def in_lists(w, h, slip):
    if (w, h, slip) not in _inl:
        _inl[(w, h, slip)] = ocn.in_lists_of(oracle_lists(w, h, slip))
    return _inl[(w, h, slip)]


def restate(w, h, slip, A, B, c, theta=THETA, **kw):
    lists = oracle_lists(w, h, slip)
    return ocn.occupancy(lists, starts_of(w, h, slip), A, B, c, theta, features=features_of(lists[0].shape[0]),
                         inl=in_lists(w, h, slip), **kw)


def restated(w, h, slip):
    """{(i, j): the restatement's dict of that pair} for the pairs of SAMPLE, computed once per pitch"""
    if (w, h, slip) not in _want:
        A, B = sets(w, h, slip)
        r = restate(w, h, slip, A, B, C_OF[(w, h, slip)], pairs=[i * NB + j for i, j in SAMPLE])
        _want[(w, h, slip)] = {ij: {k: r[k][n] for k in KEYS} for n, ij in enumerate(SAMPLE)}
    return _want[(w, h, slip)]


def full_7x67(w, h, slip):
    """(A, B, the uncapped 7 x 67 result with everything asked for) on a handle of its own, computed once"""
    if (w, h, slip) not in _full:
        A, B = sets(w, h, slip, 7, 67)
        b = SoccerBatch(1, w, h, slip)
        _full[(w, h, slip)] = (A, B, b.occupancy(A, B, THETA, C, features=features_of(b.nS), values=True))
        b.close()
    return _full[(w, h, slip)]


def same_result(got, want, what, keys=None):
    if keys is None:
        assert sorted(got) == sorted(want), (sorted(got), sorted(want))
        keys = sorted(want)
    for k in keys:
        same_bits(got[k], want[k], "%s of %s" % (k, what))


def derived(r):
    """visit_share is what the dict says it is"""
    same_bits(r["visit_share"], r["occupancy"] / r["length"][:, :, None], "visit_share")
    assert r["iterations"].dtype == np.int64


# ---- 1. every shape against the restatement, and per-lane stopping -----------------------------------------------------------
@pytest.mark.parametrize("w,h,slip", PITCHES)
def test_sampled_pairs_of_every_shape_are_the_restatement_s_bits(w, h, slip):
    want, c = restated(w, h, slip), C_OF[(w, h, slip)]
    b = SoccerBatch(1, w, h, slip)
    assert kickoff_states(b) == starts_of(w, h, slip)
    F = features_of(b.nS)
    for n_a, n_b in SHAPES:
        A, B = sets(w, h, slip, n_a, n_b)
        got = b.occupancy(A, B, THETA, c, features=F, values=True)
        assert sorted(got) == ["expect", "iterations", "length", "occupancy", "visit_share"]
        assert got["length"].shape == got["iterations"].shape == (n_a, n_b)
        assert got["expect"].shape == (n_a, n_b, N_F) and got["occupancy"].shape == (n_a, n_b, b.nS)
        derived(got)
        inside = [(i, j) for i, j in SAMPLE if i < n_a and j < n_b]
        print("%dx%d slip %.1f, %d x %d: %d of %d pairs restated" % (w, h, slip, n_a, n_b, len(inside), n_a * n_b))
        assert (0, 0) in inside and (n_a - 1, n_b - 1) in inside
        for i, j in inside:
            for k in KEYS:
                same_bits(got[k][i, j], want[(i, j)][k], "%s of pair (%d, %d) of %d x %d" % (k, i, j, n_a, n_b))
        assert (got["occupancy"][:, :, 0] == 0).all() and not np.signbit(got["occupancy"][:, :, 0]).any()
        assert (got["occupancy"] >= 0).all() and (got["length"] >= 1.0 - 1e-12).all()
    # (the last shape is 7 x 67) per-lane stopping: within one wave of 64 pairs the sweep counts are more than a full host
    # batch of 16 apart, and the pair index i changes inside a wave
    assert (n_a, n_b) == (7, 67) and len(inside) == 9                       # (3 x 5's two lie in it as well)
    it = got["iterations"].reshape(-1)
    spread = [int(it[p:p + 64].max() - it[p:p + 64].min()) for p in range(0, it.size, 64)]
    print("%dx%d slip %.1f, 7 x 67 at c = %.1f: sweeps %d .. %d, spread per wave of 64 pairs %s" % (w, h, slip, c, it.min(), it.max(), spread))
    assert len(spread) == 8 and (max(spread) > 16 or c != C)
    # a single [nS, 5] policy is a batch of one, a single [nS] feature a set of one
    one = b.occupancy(A[2], B[5], THETA, c, features=F[1], values=True)
    assert one["length"].shape == (1, 1) and one["expect"].shape == (1, 1, 1)
    same_bits(one["expect"][:, :, 0], got["expect"][2:3, 5:6, 1], "a single feature")
    same_result(one, {k: got[k][2:3, 5:6] for k in got}, "a single pair", keys=("length", "iterations", "occupancy", "visit_share"))
    b.close()


# ---- 2. passes and cached buffers -------------------------------------------------------------------------------------------
def test_no_result_depends_on_the_passes_or_on_what_the_buffers_held():
    w, h, slip = 5, 4, 0.2
    A, B, want = full_7x67(w, h, slip)
    b = SoccerBatch(1, w, h, slip)
    F = features_of(b.nS)
    small_first = b.occupancy(A[:3], B[:5], THETA, C, features=F, values=True)        # (buffers for 64 pairs, regrown below)
    for ppp in (64, 128, 448, 0):
        same_result(b.occupancy(A, B, THETA, C, features=F, values=True, pairs_per_pass=ppp), want, "7 x 67 with pairs_per_pass = %d" % ppp)
    same_result(b.occupancy(A[:3], B[:5], THETA, C, features=F, values=True), small_first, "3 x 5 after 7 x 67, against a fresh handle's")
    same_result(small_first, {k: want[k][:3, :5] for k in want}, "3 x 5 as a corner of 7 x 67")
    # after a call that failed: at the cap, and refused
    with pytest.raises(RuntimeError, match="469 of 469 pairs had not converged after max_sweeps = 3"):
        b.occupancy(A, B, THETA, C, max_sweeps=3, pairs_per_pass=128)
    with pytest.raises(AssertionError, match="pairs_per_pass"):
        b.occupancy(A, B, THETA, C, pairs_per_pass=63)
    same_result(b.occupancy(A, B, THETA, C, features=F, values=True, pairs_per_pass=64), want, "7 x 67 after two failed calls")
    b.close()


# ---- 3. what is not asked for is an extra, and the finish kernel's sums ------------------------------------------------------
def test_the_other_outputs_do_not_depend_on_what_is_asked_for_and_the_sums_are_sequential():
    w, h, slip = 5, 4, 0.2
    A, B, want = full_7x67(w, h, slip)
    b = SoccerBatch(1, w, h, slip)
    F = features_of(b.nS)
    got = b.occupancy(A, B, THETA, C)
    assert sorted(got) == ["expect", "iterations", "length"] and got["expect"].shape == (7, 67, 0)
    same_result(got, want, "7 x 67 without values or features", keys=("length", "iterations"))
    same_result(b.occupancy(A, B, THETA, C, features=F), want, "7 x 67 without values", keys=("length", "expect", "iterations"))
    same_result(b.occupancy(A, B, THETA, C, values=True), want, "7 x 67 without features", keys=("length", "iterations", "occupancy", "visit_share"))
    # a subset of the features, in another order
    sub = b.occupancy(A, B, THETA, C, features=F[[2, 0]])
    same_bits(sub["expect"], want["expect"][:, :, [2, 0]], "expect of features 2 and 0")
    # the C call with every output NULL but one
    for key in ("length", "iterations"):
        out = np.zeros((7, 67), np.float64 if key == "length" else np.int32)
        ptr = [None, None, None, None]
        ptr[0 if key == "length" else 3] = out.ctypes.data
        b._check(b.lib.soccer_occupancy(b.h, 7, A.ctypes.data, 67, B.ctypes.data, THETA, C, 1000000, 0, N_F, F.ctypes.data, *ptr))
        same_bits(out.astype(want[key].dtype), want[key], key + " alone")
    b.close()
    # length and expect are the sequential sums over the returned occupancy
    D = want["occupancy"]
    same_bits(want["length"], ocn.sequential_sum(D), "length from the occupancy")
    for q in range(N_F):
        same_bits(want["expect"][:, :, q], ocn.sequential_sum(D * F[q]), "expect[%d] from the occupancy" % q)
    derived(want)


# ---- 4. the sweep cap -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta", [THETA, 1e-3])
def test_the_sweep_cap_marks_the_open_pairs_and_keeps_their_last_iterate(theta):
    """theta = 1e-10 leaves every pair open at these caps; at theta = 1e-3 the pairs stop in between"""
    w, h, slip = 5, 4, 0.2
    A, B = sets(w, h, slip, 3, 5)
    # each pair's sweeps, as far as the caps ask: a pair still open after 34 is open at every cap
    free = restate(w, h, slip, A, B, C, theta, max_sweeps=34)["iterations"]
    print("theta %g: sweeps of the 3 x 5 pairs, 34 for more\n%s" % (theta, free))
    b = SoccerBatch(1, w, h, slip)
    F = features_of(b.nS)
    for cap in (1, 16, 17, 33):
        want = restate(w, h, slip, A, B, C, theta, max_sweeps=cap)
        late = free > cap
        if not late.any():
            got = b.occupancy(A, B, theta, C, features=F, values=True, max_sweeps=cap)
        else:
            with pytest.raises(RuntimeError, match="%d of 15 pairs had not converged after max_sweeps = %d" % (late.sum(), cap)) as e:
                b.occupancy(A, B, theta, C, features=F, values=True, max_sweeps=cap)
            got = e.value.results
        same_bits(got["iterations"], np.where(late, cap, free), "iterations at a cap of %d" % cap)
        same_result(got, want, "the 3 x 5 matrix at a cap of %d" % cap, keys=KEYS)
        derived(got)
    assert (free > 33).all() if theta == THETA else True
    b.close()


def test_a_pair_that_never_moves_stays_at_kick_off():
    b = SoccerBatch(1, 5, 4, 0.0)
    starts = kickoff_states(b)
    other = np.setdiff1d(np.arange(b.nS), starts)
    for cap in (1, 16, 17, 33, 37):
        with pytest.raises(RuntimeError, match="1 of 1 pairs had not converged") as e:
            b.occupancy(noop(b.nS), noop(b.nS), THETA, 1.0, values=True, max_sweeps=cap)
        r = e.value.results
        assert r["length"][0, 0] == float(cap) and r["iterations"][0, 0] == cap
        assert (r["occupancy"][0, 0, starts] == cap / len(starts)).all() and (r["occupancy"][0, 0, other] == 0).all()
    b.close()


# ---- 5. against match outcomes and cross-play ---------------------------------------------------------------------------------
def test_the_sum_is_the_game_length_and_the_reward_weighted_sum_is_the_payoff():
    w, h, slip = 5, 4, 0.2
    A, B, r = full_7x67(w, h, slip)
    b = SoccerBatch(1, w, h, slip)
    length = b.match_outcomes(A, B, THETA, C)["length"]
    payoff = b.cross_play(A, B, THETA, C)[0]
    nS = b.nS
    b.close()
    bound = l1_bound(nS, THETA, C) + sup_bound(THETA, C)
    gap = np.abs(r["length"] - length).max()
    print("max |sum D - length| %.3g (bound %.3g)" % (gap, bound))
    assert gap <= bound
    Pp, Pn, Pr, Pd = oracle_lists(w, h, slip)
    ER = (Pp * Pr).sum(2).reshape(nS, 5, 5)
    rbar = np.einsum("isa,jsb,sab->ijs", A, B, ER)
    gap = np.abs((r["occupancy"][:, :, 1:] * rbar[:, :, 1:]).sum(2) - payoff).max()
    print("max |sum D * r - payoff| %.3g (bound %.3g)" % (gap, bound))
    assert gap <= bound and np.abs(payoff).max() > 0.01


# ---- 6. refusals and side effects -------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    uni = np.full((761, 5), 0.2)
    one = SoccerSimultaneousEnv(width=5, height=4, player_b_policy=[0] * 761)
    with pytest.raises(AssertionError, match="two-player"):
        pl.occupancy(one, uni, uni, THETA, C)
    with pytest.raises(AssertionError, match="two-player handle"):
        one._batch.occupancy(uni, uni, THETA, C)
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=True)
    for n in (0, 1025):
        many = np.full((n, 761, 5), 0.2)
        with pytest.raises(AssertionError, match="must be 1 .. 1024, not %d and 1" % n):
            b.occupancy(many, uni, THETA, C)
        with pytest.raises(AssertionError, match="must be 1 .. 1024, not 1 and %d" % n):
            b.occupancy(uni, many, THETA, C)
    for ppp in (63, -64):
        with pytest.raises(AssertionError, match="pairs_per_pass must be 0 .* or a positive multiple of 64, not %d" % ppp):
            b.occupancy(uni, uni, THETA, C, pairs_per_pass=ppp)
    for c in (1.5, -0.1, float("nan")):
        with pytest.raises(AssertionError, match="continue_prob"):
            b.occupancy(uni, uni, THETA, c)
    with pytest.raises(AssertionError, match="max_sweeps"):
        b.occupancy(uni, uni, THETA, C, max_sweeps=0)
    with pytest.raises(AssertionError, match="theta"):
        b.occupancy(uni, uni, -1.0, C)
    with pytest.raises(AssertionError, match="the number of features must be 0 .. 16, not 17"):
        b.occupancy(uni, uni, THETA, C, features=np.ones((17, 761)))
    assert b.occupancy(uni, uni, THETA, C, features=np.ones((16, 761)))["expect"].shape == (1, 1, 16)
    with pytest.raises(AssertionError, match="features must be"):
        b.occupancy(uni, uni, THETA, C, features=np.ones((2, 760)))
    for bad, msg in ((-0.1, "negative or not a number"), (0.1, "does not sum to 1")):
        pol = np.full((3, 761, 5), 0.2)
        pol[1, 37, 2] = bad                                            # (0.1: the row sums to 0.9)
        with pytest.raises(AssertionError, match=r"soccer_occupancy: pi_a\[1\]\[37\].*" + msg):
            b.occupancy(pol, np.full((2, 761, 5), 0.2), THETA, C)
        with pytest.raises(AssertionError, match=r"soccer_occupancy: pi_b\[1\]\[37\].*" + msg):
            b.occupancy(np.full((2, 761, 5), 0.2), pol, THETA, C)
    # row 0 is not read
    pol = np.full((2, 761, 5), 0.2)
    want = b.occupancy(pol, pol, THETA, C, values=True)
    pol[:, 0] = np.nan
    same_result(b.occupancy(pol, pol, THETA, C, values=True), want, "a matrix with another row 0")
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
        b.occupancy(A, B, THETA, C)
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
            feats = pl.pitch_features(env)
            F = np.stack([feats["possession_a"], feats["ball_col"]])
            r = env.occupancy(A2, B2, THETA, C, features=F, values=True)
            same_result(pl.occupancy(env, A2, B2, THETA, C, features=F, values=True), r, "planners.occupancy against the environment's")
            # possession_a + possession_b is 1 at every state but 0, so the two shares add up to the length
            both = env.occupancy(A2, B2, THETA, C, features=feats["possession_a"] + feats["possession_b"])
            assert np.abs(both["expect"][:, :, 0] - both["length"]).max() <= 1e-12
            assert (r["expect"][:, :, 0] > 0).all() and (r["expect"][:, :, 0] < r["length"]).all()
            # a league collapsed against an opponent visits the states its mixture visits
            sigma, m = pl.collapse_mixture(env, A2, [0.5, 0.3, 0.2], 0, B2[1], 1e-14, 0.5)
            again = env.occupancy(sigma, B2[1], 1e-14, 0.5, values=True)["occupancy"][0, 0]
            gap = np.abs(again - m).sum()
            print("collapse on the device: |D_sigma - sum w D_k|_1 %.3g (bound %.3g)" % (gap, 2 * l1_bound(761, 1e-14, 0.5)))
            assert gap <= 2 * l1_bound(761, 1e-14, 0.5)
            with pytest.raises(RuntimeError, match="had not converged"):
                env.occupancy(A2, B2, THETA, C, max_sweeps=3)
            with pytest.raises(AssertionError, match="pairs_per_pass"):
                env.occupancy(A2, B2, THETA, C, pairs_per_pass=65)
            assert env.batch.tick == tick
        O, R, TE, TR, _ = env.rollout(20, sample_actions=True)
        outs.append((O["player_a"].copy(), R["player_a"].copy(), TE["player_a"].copy(), TR["player_a"].copy()))
        env.close()
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x, y)


# ---- 7. populations ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["q", "wolf", "minimax_q", "om"])
def test_a_population_s_occupancy_is_the_batch_s_on_what_read_returns(kind):
    n = 67
    make = {"q": lambda b, g: b.q_population(g), "wolf": lambda b, g: b.wolf_population(g),
            "minimax_q": lambda b, g: b.minimax_q_population(g), "om": lambda b, g: b.om_population(g)}[kind]
    b = SoccerBatch(n, 5, 4, 0.2, seed=7, autoreset=True)
    F = features_of(b.nS)
    pop = make(b, C)
    b.reset(); pop.run(40)
    r = pop.read()
    got = pop.occupancy(features=F)
    assert got["length"].shape == (n, n) and got["expect"].shape == (n, n, N_F) and "occupancy" not in got
    same_result(got, b.occupancy(r["pi_a"], r["pi_b"], THETA, C, features=F), "the population's matrix")
    part = pop.occupancy(first=1, count=3, continue_prob=0.5, theta=1e-8, values=True)
    same_result(part, b.occupancy(r["pi_a"][1:4], r["pi_b"][1:4], 1e-8, 0.5, values=True), "members 1 .. 3 at another continuation probability")
    if kind == "wolf":
        same_result(pop.occupancy(which="avg"), b.occupancy(r["avg_a"], r["avg_b"], THETA, C), "the average policies' matrix")
    if kind == "om":
        same_result(pop.occupancy("model"), b.occupancy(r["model_a"], r["model_b"], THETA, C), "the models' matrix")
    pop.close()
    gam = np.full(n, 0.9); gam[2] = 0.8
    mixed = make(b, gam)
    with pytest.raises(ValueError, match="members 0 and 2 have different discounts .* pass continue_prob"):
        mixed.occupancy()
    assert mixed.occupancy(count=2)["length"].shape == (2, 2)                   # members 0 and 1 share theirs
    assert mixed.occupancy(first=1, count=3, continue_prob=0.9)["length"].shape == (3, 3)
    mixed.close(); b.close()


# ---- 8. a large pitch -------------------------------------------------------------------------------------------------------
def test_a_large_pitch():
    """c = 0.5: sweep k moves no state by more than 0.5^(k-1), so every pair stops within 35 sweeps"""
    w, h, slip, c = 11, 7, 0.2, 0.5
    A, B = policy_set(w, h, slip, 2, 31), policy_set(w, h, slip, 3, 32)
    b = SoccerBatch(1, w, h, slip)
    assert b.nS == 11705
    got = b.occupancy(A, B, THETA, c, features=features_of(b.nS), values=True)
    b.close()
    print("11x7: length %s sweeps %s" % (np.round(got["length"], 6).tolist(), got["iterations"].tolist()))
    assert got["iterations"].max() <= 35
    flat = [0, 4, 5]                                                    # 3 of the 6 pairs: the first, one of each row, the last
    want = restate(w, h, slip, A, B, c, pairs=flat)
    for n, f in enumerate(flat):
        for k in KEYS:
            same_bits(got[k][f // 3, f % 3], want[k][n], "%s of pair %d" % (k, f))
