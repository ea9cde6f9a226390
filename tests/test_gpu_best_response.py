"""Best responses to mixed policies on the device (soccer_best_response, soccer_evaluate_policies): bit for bit the numpy
restatement over the CPU oracle's lists (tests/best_response_np.py), every policy of a batch to the bits and the sweep count
it has alone, the existing single-agent planner recovered from one-hot policies, the three modes consistent with one
another, the equilibrium strategies unexploitable, the learner's strategy harder and harder to beat, and the refusals."""
import os
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch, SoccerSimultaneousEnv, VectorSoccerEnv
from gym_soccer_littman94_amd import planners as pl
from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_response_np as brn  # noqa: E402
from minimax_q_np import shapley_lists  # noqa: E402
from test_gpu_minimax import facade, host_q, sigma_index  # noqa: E402

pytestmark = pytest.mark.gpu

GAMMA, THETA = 0.9, 1e-10
PITCHES = [(5, 4, 0.0), (5, 4, 0.2), (7, 5, 0.3)]

_lists, _star = {}, {}


def oracle_lists(w, h, slip):
    if (w, h, slip) not in _lists:
        _lists[(w, h, slip)] = shapley_lists(Oracle(w, h, slip, n=1, seed=0))
    return _lists[(w, h, slip)]


def minimax(w, h, slip):
    """(pi_a, pi_b, V*) of minimax value iteration on the device"""
    if (w, h, slip) not in _star:
        b = SoccerBatch(1, w, h, slip)
        _star[(w, h, slip)] = b.minimax_value_iteration(THETA, GAMMA)[:3]
        b.close()
    return _star[(w, h, slip)]


def policies(w, h, slip, seed=11):
    """uniform, the two minimax strategies, Dirichlet rows (two concentrations), one-hot rows: [6, nS, 5]"""
    pa, pb, _ = minimax(w, h, slip)
    nS = pa.shape[0]
    rng = np.random.default_rng(seed)
    return np.stack([np.full((nS, 5), 0.2), pa, pb, rng.dirichlet(np.ones(5), nS), rng.dirichlet(np.full(5, 0.2), nS),
                     brn.onehot(rng.integers(0, 5, nS))])


def same_bits(got, want, what):
    g = np.ascontiguousarray(got); w = np.ascontiguousarray(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if g.dtype == np.float64:
        g = g.view(np.int64); w = np.ascontiguousarray(w, np.float64).view(np.int64)
    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    assert bad.size == 0, "%s differs in %d entries, first at flat index %d: %r vs %r" % (
        what, bad.size, bad[0], np.asarray(got).reshape(-1)[bad[0]], np.asarray(want).reshape(-1)[bad[0]])


def capped(call):
    """the results of a solve that stops at max_sweeps (RuntimeError.results), or of one that converges"""
    try:
        return call(), False
    except RuntimeError as e:
        assert "had not converged" in str(e)
        return e.results, True


# ---- 1. bit equality with the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,slip", PITCHES)
def test_bit_identical_to_the_numpy_restatement(w, h, slip):
    lists = oracle_lists(w, h, slip)
    pol = policies(w, h, slip)
    b = SoccerBatch(1, w, h, slip)
    for player in (0, 1):
        br, V, Qr, it = b.best_response(pol, player, THETA, GAMMA)
        wbr, wV, wQr, wit = brn.best_response(lists, pol, player, GAMMA, THETA)
        print("%dx%d slip %.1f, response to player %s's policies: sweeps %s" % (w, h, slip, "AB"[player], it.tolist()))
        same_bits(V, wV, "V"); same_bits(Qr, wQr, "Qr"); same_bits(br, wbr, "br"); same_bits(it, wit, "iterations")
        assert (it <= 220).all() and br.dtype == np.int64 and (V[:, 0] == 0).all()
    other = np.roll(pol, 1, axis=0)
    V, it = b.evaluate_policies(pol, other, THETA, GAMMA)
    wV, wit = brn.evaluate(lists, pol, other, GAMMA, THETA)
    same_bits(V, wV, "V of the pairs"); same_bits(it, wit, "iterations of the pairs")
    # a single policy: no leading axis comes back, and one policy meets every policy of a batch
    br1, V1, Qr1, it1 = b.best_response(pol[3], 0, THETA, GAMMA)
    assert br1.shape == (b.nS,) and V1.shape == (b.nS,) and Qr1.shape == (b.nS, 5) and isinstance(it1, int)
    Vp, itp = b.evaluate_policies(pol[1], pol, THETA, GAMMA)
    wVp, witp = brn.evaluate(lists, np.broadcast_to(pol[1], pol.shape), pol, GAMMA, THETA)
    same_bits(Vp, wVp, "V of one policy against a batch"); same_bits(itp, witp, "its iterations")
    V2, it2 = b.evaluate_policies(pol[1], pol[2], THETA, GAMMA)
    assert V2.shape == (b.nS,) and isinstance(it2, int)
    same_bits(V2, Vp[2], "V of a single pair")
    b.close()


@pytest.mark.parametrize("w,h,slip", PITCHES)
def test_q_behind_the_sums_is_the_host_sum_over_the_facade_lists(w, h, slip):
    """Against the constant policy 'always a' the five sums are row a of Q itself (the other four terms add zeros), so five
    constant policies per side show all of Q_k = Q(V_{k-1}), with V_{k-1} what a solve capped one sweep earlier returns."""
    env, lists = facade(w, h, slip)
    b = SoccerBatch(1, w, h, slip)
    const = np.stack([brn.onehot(np.full(b.nS, a)) for a in range(5)])
    m = 7
    for player in (0, 1):
        (_, Vm, _, itm), stopped = capped(lambda: b.best_response(const, player, THETA, GAMMA, max_sweeps=m))
        assert stopped and (itm == m).all()
        (_, _, Qr, _), _ = capped(lambda: b.best_response(const, player, THETA, GAMMA, max_sweeps=m + 1))
        for a in range(5):
            Q = host_q(lists, Vm[a], GAMMA)
            same_bits(Qr[a], Q[:, a, :] if player == 0 else Q[:, :, a], "Q of the constant policy %d" % a)
    b.close()


# ---- 2. batch independence ---------------------------------------------------------------------------------------------
def test_every_policy_of_a_batch_solves_as_it_does_alone():
    w, h, slip = 5, 4, 0.2
    pol = policies(w, h, slip)
    pol = np.concatenate([pol, pol[:2]])                                  # uniform and the minimax strategy once more, at the end
    b = SoccerBatch(1, w, h, slip)
    for player in (0, 1):
        alone = [b.best_response(p, player, THETA, GAMMA) for p in pol]    # (also: a batch of 1 first, larger ones after it)
        both = b.best_response(pol, player, THETA, GAMMA)
        ks = both[3]
        print("sweeps per policy (player %s held fixed): %s" % ("AB"[player], ks.tolist()))
        assert ks.min() + 40 < ks.max(), "the batch should mix easy and hard policies"
        for i in range(len(pol)):
            for name, x, y in zip(("br", "V", "Qr"), both, alone[i]):
                same_bits(x[i], y, "%s of policy %d" % (name, i))
            assert ks[i] == alone[i][3]
        # max_sweeps not a multiple of the 16 sweeps between two synchronisations: the same results
        again = b.best_response(pol, player, THETA, GAMMA, max_sweeps=int(ks.max()) + (1 if (ks.max() + 1) % 16 else 2))
        for name, x, y in zip(("br", "V", "Qr", "iterations"), again, both):
            same_bits(x, y, name)
        # too few sweeps for some: those report max_sweeps and hold their last iterate, the rest are complete
        m = int(ks.min()) + 5
        m += 0 if m % 16 else 1
        res, stopped = capped(lambda: b.best_response(pol, player, THETA, GAMMA, max_sweeps=m))
        assert stopped
        late = ks > m
        assert late.any() and (~late).any()
        assert (res[3][late] == m).all() and (res[3][~late] == ks[~late]).all()
        for name, x, y in zip(("br", "V", "Qr"), res, both):
            same_bits(x[~late], y[~late], name + " of the policies that converged")
        wbr, wV, wQr, wit = brn.best_response(oracle_lists(w, h, slip), pol, player, GAMMA, THETA, max_sweeps=m)
        same_bits(res[1], wV, "V at max_sweeps"); same_bits(res[2], wQr, "Qr at max_sweeps"); same_bits(res[3], wit, "iterations")
    # pairs likewise
    other = np.roll(pol, 3, axis=0)
    V, ks = b.evaluate_policies(pol, other, THETA, GAMMA)
    for i in range(len(pol)):
        Vi, ki = b.evaluate_policies(pol[i], other[i], THETA, GAMMA)
        same_bits(V[i], Vi, "V of pair %d" % i)
        assert ks[i] == ki
    b.close()


# ---- 3. agreement with the single-agent planner --------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,slip", PITCHES)
def test_one_hot_policies_give_the_single_agent_planner_s_answer(w, h, slip):
    """The single-agent list P[s][a] is the two-player list P[s][(a, pol[s])] (learner B: with the reward negated), and a
    one-hot sum adds only zeros: V_k = max_a Q, br = pi and the sweep count of soccer_value_iteration, exactly."""
    b = SoccerBatch(1, w, h, slip)
    nS = b.nS
    pol = np.random.default_rng(23).integers(0, 5, nS)
    # B is fixed, A learns
    one = SoccerSimultaneousEnv(width=w, height=h, slip_prob=slip, player_b_policy=pol.tolist())
    pi, _, Q, k = pl.value_iteration(one, THETA, GAMMA)
    br, V, Qr, it = b.best_response(brn.onehot(pol), 1, THETA, GAMMA)
    assert it == k
    assert np.array_equal(V[1:], Q.max(1)[1:]) and np.array_equal(br[1:], pi[1:]) and np.array_equal(Qr[1:], Q[1:])
    # A is fixed, B learns: its table holds -r, so its values are the negated ones and its maximum is A's minimum
    one = SoccerSimultaneousEnv(width=w, height=h, slip_prob=slip, player_a_policy=pol.tolist())
    pi, _, Q, k = pl.value_iteration(one, THETA, GAMMA)
    br, V, Qr, it = b.best_response(brn.onehot(pol), 0, THETA, GAMMA)
    assert it == k
    assert np.array_equal(V[1:], -Q.max(1)[1:]) and np.array_equal(br[1:], pi[1:]) and np.array_equal(Qr[1:], -Q[1:])
    b.close()


# ---- 4. the three modes agree --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,slip", PITCHES)
def test_a_policy_against_its_best_response_has_the_response_value(w, h, slip):
    pol = policies(w, h, slip)
    b = SoccerBatch(1, w, h, slip)
    bound = 2 * GAMMA * THETA / (1 - GAMMA) + 1e-12        # both are theta-converged iterates of one contraction
    br, V, _, _ = b.best_response(pol, 0, THETA, GAMMA)
    Ve, _ = b.evaluate_policies(pol, brn.onehot(br), THETA, GAMMA)
    d0 = np.abs(Ve - V).max()
    br, V, _, _ = b.best_response(pol, 1, THETA, GAMMA)
    Ve, _ = b.evaluate_policies(brn.onehot(br), pol, THETA, GAMMA)
    d1 = np.abs(Ve - V).max()
    print("%dx%d slip %.1f: |evaluate(x, br) - response| %.3g, |evaluate(br, y) - response| %.3g, bound %.3g" % (w, h, slip, d0, d1, bound))
    assert d0 <= bound and d1 <= bound
    b.close()


# ---- 5. equilibrium --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,slip", PITCHES + [(11, 7, 0.2)])
def test_the_minimax_strategies_cannot_be_exploited(w, h, slip):
    env = SoccerSimultaneousEnv(width=w, height=h, slip_prob=slip)
    pa, pb, vstar, _, _ = pl.minimax_value_iteration(env, THETA, GAMMA)
    r = pl.exploitability(env, pa, pb, THETA, GAMMA)
    gap = r["gap"][1:]
    print("%dx%d slip %.1f: max gap %.3g, max (V* - v_a) %.3g, max (v_b - V*) %.3g, sweeps %s" % (
        w, h, slip, gap.max(), (vstar - r["v_a"])[1:].max(), (r["v_b"] - vstar)[1:].max(), r["iterations"]))
    assert gap.shape == (env.nS - 1,) and (gap <= 2e-6).all()
    assert (r["v_a"][1:] >= vstar[1:] - 1e-6).all() and (r["v_b"][1:] <= vstar[1:] + 1e-6).all()
    assert r["br_a"].shape == r["br_b"].shape == (env.nS,)
    # the uniform policy next to them, as a batch on one side only
    both = pl.exploitability(env, np.stack([pa, np.full(pa.shape, 0.2)]), pb, THETA, GAMMA)
    assert both["gap"].shape == (2, env.nS)
    same_bits(both["gap"][0], r["gap"], "the gap of the minimax pair")
    alone = pl.best_response(env, np.full(pa.shape, 0.2), 0, THETA, GAMMA)[1]
    same_bits(both["v_a"][1], alone, "the uniform policy's worst case")
    same_bits(both["gap"][1], r["v_b"] - alone, "the gap of (uniform, pi_b)")
    # no policy's worst case lies above the game's value, which pi_b's worst case meets within 1e-6 (above)
    print("    (uniform, pi_b): max gap %.3g, min gap %.3g" % (both["gap"][1, 1:].max(), both["gap"][1, 1:].min()))
    assert (both["gap"][1, 1:] >= -2e-6).all()
    if (w, h) == (5, 4):
        # uniform on both sides: the restatement measured a maximum gap of 1.46 (slip 0) and 1.26 (slip 0.2) on this pitch
        uni = pl.exploitability(env, np.full(pa.shape, 0.2), np.full(pa.shape, 0.2), THETA, GAMMA)
        print("    (uniform, uniform): max gap %.3g" % uni["gap"][1:].max())
        assert uni["gap"][1:].max() > 1.0


@pytest.mark.parametrize("w,h,slip", PITCHES)
def test_mirror_antisymmetry_of_response_values(w, h, slip):
    """v_a(pi)[s] = -v_b(sigma pi)[sigma s]: sigma swaps the players and reflects the columns (EAST <-> WEST)"""
    env, _ = facade(w, h, slip)
    sig = sigma_index(env)
    act = np.array([0, 1, 2, 4, 3])
    pol = policies(w, h, slip)[[1, 3]]                                    # the minimax strategy of A and Dirichlet rows
    mirrored = np.full(pol.shape, 0.2)
    mirrored[:, sig[1:]] = pol[:, 1:][:, :, act]
    v_a = pl.best_response(env, pol, 0, THETA, GAMMA)[1]
    v_b = pl.best_response(env, mirrored, 1, THETA, GAMMA)[1]
    gap = np.abs(v_a[:, 1:] + v_b[:, sig[1:]]).max()
    print("%dx%d slip %.1f: mirror gap of response values %.3g" % (w, h, slip, gap))
    assert gap <= 2 * THETA / (1 - GAMMA)
    assert np.abs(v_a).max() > 0.01


# ---- 6. the learner learns to be hard to beat ----------------------------------------------------------------------------
def test_the_learner_s_strategy_gets_harder_to_beat():
    """The run of test_it_learns_the_minimax_values (5x4, slip 0, 65 536 lanes x 3 000 steps, seed 1994, Q0 = 0, uniform B),
    its pi_a at 0 / 100 / 500 / 1 500 / 3 000 steps solved as one batch.  The numpy learner, which the device learner is
    pinned to bit for bit, gave mean over live states of V* - v_a: 0.6006, 0.0474, 0.0405, 0.0153, 0.00273 and a maximum of
    0.0401 at 3 000 steps; the bounds below leave the margin that test's 0.07 leaves its 0.0249."""
    n, T = 65536, 3000
    marks = [0, 100, 500, 1500, 3000]
    env = VectorSoccerEnv(n, 5, 4, 0.0, seed=1994, autoreset=True)
    vstar = pl.minimax_value_iteration(env, THETA, GAMMA)[2]
    obs0, _ = env.reset()
    starts = np.unique(obs0["player_a"])
    q = env.minimax_q(GAMMA, alpha=1.0, decay=0.01 ** (1.0 / T), explor=0.2, q_init=0.0, opponent="uniform")
    snaps, done = [], 0
    for m in marks:
        if m > done:
            q.run(m - done); done = m
        snaps.append(q.pi_a)
    _, v_a, _, it = pl.best_response(env, np.stack(snaps), 0, THETA, GAMMA)
    short = (vstar - v_a)[:, 1:]
    for m, d, v, k in zip(marks, short, v_a, it):
        print("after %4d steps: V* - v_a mean %.5f max %.5f (%3d sweeps); worst case at the initial states %s (V* %s)" % (
            m, d.mean(), d.max(), k, np.round(v[starts], 4).tolist(), np.round(vstar[starts], 4).tolist()))
    assert (short >= -1e-6).all(), "no policy can have a worst case above the game's value"
    assert short[-1].mean() <= 0.01 and short[-1].max() <= 0.10
    assert short[-1].mean() < short[1].mean()
    # the learner's own call: the same solve of what it holds now
    r = q.exploitability(THETA)
    same_bits(r["v_a"], v_a[-1], "v_a of MinimaxQLearner.exploitability")
    assert r["gap"].shape == (env.nS,) and (r["gap"][1:] >= -1e-6).all()
    q.close(); env.close()


# ---- 7. refusals and side effects ----------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    uni = np.full((761, 5), 0.2)
    one = SoccerSimultaneousEnv(width=5, height=4, player_b_policy=[0] * 761)
    with pytest.raises(AssertionError, match="two-player"):
        pl.best_response(one, uni, 0, THETA, GAMMA)
    with pytest.raises(AssertionError, match="two-player"):
        pl.exploitability(one, uni, uni, THETA, GAMMA)
    with pytest.raises(AssertionError, match="two-player handle"):
        one._batch.best_response(uni, 0, THETA, GAMMA)
    with pytest.raises(AssertionError, match="two-player handle"):
        one._batch.evaluate_policies(uni, uni, THETA, GAMMA)
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=True)
    for gamma in (1.5, -0.1, float("nan")):
        with pytest.raises(AssertionError, match="discount_factor"):
            b.best_response(uni, 0, THETA, gamma)
        with pytest.raises(AssertionError, match="discount_factor"):
            b.evaluate_policies(uni, uni, THETA, gamma)
    for n in (0, 257):
        with pytest.raises(AssertionError, match="number of policies must be 1 .. 256, not %d" % n):
            b.best_response(np.full((n, 761, 5), 0.2), 1, THETA, GAMMA)
        with pytest.raises(AssertionError, match="number of policies"):
            b.evaluate_policies(np.full((n, 761, 5), 0.2), np.full((n, 761, 5), 0.2), THETA, GAMMA)
    with pytest.raises(AssertionError, match="max_sweeps"):
        b.best_response(uni, 0, THETA, GAMMA, max_sweeps=0)
    with pytest.raises(AssertionError, match="theta"):
        b.best_response(uni, 0, -1.0, GAMMA)
    with pytest.raises(AssertionError, match="player"):
        b.best_response(uni, 2, THETA, GAMMA)
    with pytest.raises(AssertionError, match="n_states"):
        b.best_response(np.full((760, 5), 0.2), 0, THETA, GAMMA)
    for bad, msg in ((-0.1, "negative or not a number"), (float("nan"), "negative or not a number"), (0.1, "does not sum to 1")):
        pol = np.full((3, 761, 5), 0.2)
        pol[1, 37, 2] = bad                                            # (0.1: the row sums to 0.9)
        for player in (0, 1):
            with pytest.raises(AssertionError, match=r"policy\[1\]\[37\].*" + msg):
                b.best_response(pol, player, THETA, GAMMA)
        with pytest.raises(AssertionError, match=r"pi_a\[1\]\[37\].*" + msg):
            b.evaluate_policies(pol, np.full((3, 761, 5), 0.2), THETA, GAMMA)
        with pytest.raises(AssertionError, match=r"pi_b\[1\]\[37\].*" + msg):
            b.evaluate_policies(np.full((3, 761, 5), 0.2), pol, THETA, GAMMA)
    # row 0 is not read
    pol = np.full((761, 5), 0.2)
    want = b.best_response(pol, 0, THETA, GAMMA)
    pol[0] = np.nan
    for x, y in zip(b.best_response(pol, 0, THETA, GAMMA)[:3], want[:3]):
        same_bits(x, y, "a result with another row 0")
    b.close()


def test_capture_no_ticks_layout_and_a_new_handle(monkeypatch):
    pol = policies(5, 4, 0.0)
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=True)
    want = b.best_response(pol, 0, THETA, GAMMA) + b.best_response(pol, 1, THETA, GAMMA) + b.evaluate_policies(pol, pol[::-1], THETA, GAMMA)
    # during a graph capture: refused, and the capture still completes
    b.reset()
    n = 64
    A = b.alloc(n, np.int8).fill(0); B = b.alloc(n, np.int8).fill(1)
    obs = b.alloc(n, np.uint16); rew = b.alloc(n, np.int8); term = b.alloc(n, np.uint8); trunc = b.alloc(n, np.uint8)
    b.graph_begin()
    b.step_plain(A, B, obs, rew, term, trunc)
    with pytest.raises(RuntimeError, match="graph capture"):
        b.best_response(pol, 0, THETA, GAMMA)
    with pytest.raises(RuntimeError, match="graph capture"):
        b.evaluate_policies(pol, pol, THETA, GAMMA)
    b.graph_destroy(b.graph_end())
    b.close()
    # the state layout and a destroyed and recreated handle change no bit
    for layout in ("wide", None):
        if layout:
            monkeypatch.setenv("SOCCER_STATE_LAYOUT", layout)
        b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=True)
        if layout:
            monkeypatch.delenv("SOCCER_STATE_LAYOUT")
            assert b.lib.soccer_state_streams(b.h) == 6
        got = b.best_response(pol, 0, THETA, GAMMA) + b.best_response(pol, 1, THETA, GAMMA) + b.evaluate_policies(pol, pol[::-1], THETA, GAMMA)
        for x, y in zip(got, want):
            same_bits(x, y, "a result on another handle (layout %s)" % layout)
        b.close()
    # a solve consumes no tick and leaves the lanes alone: the same rollout with and without one
    outs = []
    for solve in (False, True):
        env = VectorSoccerEnv(4096, slip_prob=0.2, seed=3)
        env.reset()
        if solve:
            tick = env.batch.tick
            uni = np.full((2, env.nS, 5), 0.2)
            pl.exploitability(env, uni, uni[0], THETA, GAMMA)
            env.batch.evaluate_policies(uni, uni, THETA, GAMMA)
            assert env.batch.tick == tick
        O, R, TE, TR, _ = env.rollout(50, sample_actions=True)
        outs.append((O["player_a"].copy(), R["player_a"].copy(), TE["player_a"].copy(), TR["player_a"].copy()))
        env.close()
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x, y)
