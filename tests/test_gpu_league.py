"""-m gpu: the league opponent of the population of Q-learners (include/soccer_hip.h, "learners, a league opponent for the
population of Q-learners") — against the populations that exist where the two must agree, device against device, and against
its numpy restatement (tests/league_np.py) bit for bit in Q_a, Q_b, alpha, steps and picks; then launch shapes, composition,
checkpoints, frozen lanes and the refusals.  Conventions of tests/test_gpu_q_population.py: its RUN_KW, its T."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch, VectorSoccerEnv, _lib
from gym_soccer_littman94_amd import planners as pl
from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from league_np import QLeagueNumpy, assert_league_equal, league_pick, league_thresholds  # noqa: E402
from philox_np import lane_words  # noqa: E402
from q_population_np import assert_population_equal  # noqa: E402
from test_population_edges_np import CASES as EDGE_CASES, G0_LEAGUE_PLAYER, KW as EDGE_KW, g0_league, reference_g0  # noqa: E402

G0 = EDGE_CASES["G0"]

pytestmark = pytest.mark.gpu

GAMMA = 0.9
SEED, T_RUN = 1994, 60
RUN_KW = dict(explor=0.2, decay=0.99)


def make_league(K, nS):
    """K mixed policies and uneven weights; from K = 5 on the first, every third and the last weight are zero"""
    rng = np.random.default_rng(100 + K)
    pol = rng.dirichlet(np.ones(5), (K, nS))
    w = rng.dirichlet(np.ones(K)) + 0.05 / K
    if K >= 5:
        w[0] = 0.0; w[2::3] = 0.0; w[-1] = 0.0
    return pol, w / w.sum()


def other_of(name, nS):
    return np.random.default_rng(11).dirichlet(np.ones(5), nS) if name == "fixed" else name


def device(K, n, player, other="greedy", w=5, h=4, slip=0.2, lane_offset=0, max_steps=5, reset=True, league=None):
    b = SoccerBatch(n, w, h, slip, seed=SEED, autoreset=True, max_steps=max_steps, lane_offset=lane_offset)
    pol, wt = make_league(K, b.nS) if league is None else league
    acts = dict(act_a="league", act_b=other_of(other, b.nS)) if player == 0 else dict(act_a=other_of(other, b.nS), act_b="league")
    q = b.q_population(GAMMA, league_policies=pol, league_weights=wt, **acts, **RUN_KW)
    assert q.league == player and q.n_policies == K
    if reset:
        b.reset()
    return b, q


def restatement(K, n, player, other="greedy", w=5, h=4, slip=0.2, lane_offset=0, max_steps=5):
    o = Oracle(w, h, slip, n=n, seed=SEED, autoreset=True, max_steps=max_steps, lane_offset=lane_offset)
    pol, wt = make_league(K, o.nS)
    return o, QLeagueNumpy(n, o.nS, GAMMA, player, pol, wt, other=other_of(other, o.nS), **RUN_KW)


_REFERENCE = {}


def reference_run(*case):
    """the restatement after T_RUN steps from a reset: computed once per case and left unchanged"""
    if case not in _REFERENCE:
        o, ref = restatement(*case)
        ref.run(o, o.reset(), T_RUN)
        _REFERENCE[case] = (o, ref)
    return _REFERENCE[case]


def read_all(q):
    r = q.read()
    r["pick"] = q.picks()
    return r


def assert_state_equal(b, o):
    s = b.get_state()
    np.testing.assert_array_equal(s["row_a"], o.row_a); np.testing.assert_array_equal(s["col_a"], o.col_a)
    np.testing.assert_array_equal(s["row_b"], o.row_b); np.testing.assert_array_equal(s["col_b"], o.col_b)
    np.testing.assert_array_equal(s["poss"], o.poss & 1)
    np.testing.assert_array_equal(s["needs_reset"], (o.poss >> 1) & 1)
    np.testing.assert_array_equal(s["t"], o.t)


def assert_batches_equal(b1, b2):
    s1, s2 = b1.get_state(), b2.get_state()
    for k in s1:
        np.testing.assert_array_equal(s1[k], s2[k])
    assert b1.tick == b2.tick
    np.testing.assert_array_equal(b1.stats()[0], b2.stats()[0])


# ---- 1. equivalence with what exists, device against device ---------------------------------------------------
@pytest.mark.parametrize("player", [0, 1])
@pytest.mark.parametrize("K", [1, 3])
def test_a_league_of_one_live_policy_is_the_shared_fixed_population(K, player):
    n = 259
    b0 = SoccerBatch(n, 5, 4, 0.2, seed=SEED, autoreset=True, max_steps=5)
    pol = np.random.default_rng(5).dirichlet(np.ones(5), (3, b0.nS))
    acts = dict(act_a=pol[1], act_b="greedy") if player == 0 else dict(act_a="greedy", act_b=pol[1])
    q0 = b0.q_population(GAMMA, **acts, **RUN_KW)
    b0.reset(); q0.run(T_RUN)
    league = (pol[1:2], np.array([1.0])) if K == 1 else (pol, np.array([0.0, 1.0, 0.0]))
    b1, q1 = device(K, n, player, league=league)
    q1.run(T_RUN)
    assert_population_equal(q1.read(), q0.read())
    assert_batches_equal(b1, b0)
    picks = q1.picks()
    assert set(picks.tolist()) <= {-1, K // 2} and (picks == -1).any() and (picks == K // 2).any()
    assert q0.league is None
    b0.close(); b1.close()


# ---- 2. the restatement, bit for bit -----------------------------------------------------------------------------
# (K, n, league player, the other player, width, height, slip, lane_offset); max_steps = 5: most episodes end by truncation
RUN_CASES = [(2, 259, 1, "greedy", 5, 4, 0.0, 0),
             (1024, 3, 0, "greedy", 5, 4, 0.2, 0),
             (5, 67, 1, "uniform", 5, 4, 0.2, 6),
             (5, 67, 0, "fixed", 7, 5, 0.3, 0),
             (5, 1, 1, "greedy", 5, 4, 0.0, 3),
             (2, 259, 0, "uniform", 5, 4, 0.2, 0),
             (1024, 3, 1, "fixed", 7, 5, 0.3, 1),
             # 12x14 at the slip of the populations' G: pop_league_run_kernel with the observation table in global memory
             (5, 17, 1, "greedy", 12, 14, 0.2, 0)]


@pytest.mark.parametrize("case", RUN_CASES, ids=lambda c: "K%d-n%d-p%d-%s-%dx%d-s%s-off%d" % c)
def test_run_equals_the_restatement_bit_for_bit(case):
    K, n, player, other, w, h, slip, off = case
    o, ref = reference_run(*case)
    b, q = device(*case)
    q.run(T_RUN)
    assert_league_equal(read_all(q), ref.state())
    assert_state_equal(b, o)
    assert b.tick == o.tick == T_RUN + 1
    hist, misuse = b.stats()
    np.testing.assert_array_equal(hist, o.hist)
    assert misuse == 0 and q.steps == T_RUN
    assert ref.n_redraws > 0 and ref.n_truncated_only > 0
    # two different picks live at once; one lane can only show two different picks one after the other
    assert (ref.max_live if n > 1 else len(ref.seen)) >= 2
    part = q.picks(n // 2, 1)
    assert part.shape == (1,) and part[0] == ref.pick[n // 2]
    b.close()


def test_run_on_12x14_without_slip_equals_the_restatement_bit_for_bit():
    """case G0 of tests/test_population_edges_np.py, which shows without a GPU that it terminates, truncates, meets s' == s
    and holds two picks at once: pop_league_run_kernel<SLIP = false, LUT_LDS = false>"""
    c = G0
    o, ref = reference_g0("league")
    assert (c["w"], c["h"], c["slip"]) == (12, 14, 0.0) and RUN_KW == EDGE_KW["q"]
    b, q = device(3, c["n"], G0_LEAGUE_PLAYER, "greedy", c["w"], c["h"], c["slip"], 0, c["max_steps"], league=g0_league(o.nS))
    q.run(c["T"])
    assert_league_equal(read_all(q), ref.state())
    assert_state_equal(b, o)
    assert b.tick == o.tick == c["T"] + 1
    hist, misuse = b.stats()
    np.testing.assert_array_equal(hist, o.hist)
    assert misuse == 0 and q.steps == c["T"]
    assert ref.n_redraws > 0 and ref.n_truncated_only > 0 and ref.n_terminated > 0 and ref.n_same > 0 and ref.max_live >= 2
    b.close()


# ---- 3. launch shape, composition ---------------------------------------------------------------------------------
def test_result_does_not_depend_on_the_steps_per_launch_or_the_grid(monkeypatch):
    case = RUN_CASES[0]
    want = reference_run(*case)[1].state()
    monkeypatch.setenv("SOCCER_POP_LAUNCH_STEPS", "7")          # slip 0: a launch starts in the middle of a Philox block
    b, q = device(*case); q.run(T_RUN)
    monkeypatch.delenv("SOCCER_POP_LAUNCH_STEPS")
    assert_league_equal(read_all(q), want)
    b.close()
    monkeypatch.setenv("SOCCER_POP_GRID_BLOCKS", "1")           # 259 members on one workgroup: a thread serves two picks
    b, q = device(*case); q.run(T_RUN)
    monkeypatch.delenv("SOCCER_POP_GRID_BLOCKS")
    assert_league_equal(read_all(q), want)
    b.close()


def test_runs_compose():
    case = RUN_CASES[5]
    b1, q1 = device(*case); q1.run(T_RUN)
    b2, q2 = device(*case); q2.run(25); q2.run(35)
    assert_league_equal(read_all(q2), read_all(q1))
    assert_batches_equal(b1, b2)
    assert_league_equal(read_all(q1), reference_run(*case)[1].state())
    b1.close(); b2.close()


# ---- 4. checkpoints --------------------------------------------------------------------------------------------
def test_read_and_picks_then_load_and_load_picks_on_a_fresh_population_continue_the_same():
    case = RUN_CASES[5]
    K, n, player, other = case[:4]
    b, q = device(*case); q.run(25)                             # an odd number of steps: most lanes are mid-episode
    ck = read_all(q)
    assert (ck["pick"] >= 0).any() and (ck["pick"] == -1).any()
    q2 = b.q_population(GAMMA, act_a="league", act_b=other, league_policies=make_league(K, b.nS)[0],
                        league_weights=make_league(K, b.nS)[1], **RUN_KW)       # a second, fresh population on the same handle
    assert (q2.picks() == -1).all()
    q2.load(ck["Q_a"], ck["Q_b"], alpha=ck["alpha"], steps=ck["steps"]).load_picks(ck["pick"])
    assert_league_equal(read_all(q2), ck)
    q2.run(35)
    assert_league_equal(read_all(q2), reference_run(*case)[1].state())
    # a range alone
    q.load_picks([1, 0, -1], first=5)
    assert q.picks(5, 3).tolist() == [1, 0, -1] and q.picks(0, 5).tolist() == ck["pick"][:5].tolist()
    b.close()


def test_load_picks_of_minus_one_forces_a_redraw_at_the_next_step():
    case = RUN_CASES[2]
    o, ref = restatement(*case)
    obs = ref.run(o, o.reset(), 25)
    b, q = device(*case); q.run(25)
    assert_league_equal(read_all(q), ref.state())
    live = ref.pick >= 0
    assert live.any()
    redraws = ref.n_redraws
    ref.pick[:] = -1
    q.load_picks(np.full(q.n, -1))
    ref.run(o, obs, 35); q.run(35)
    assert ref.n_redraws - redraws >= int(live.sum())            # the lanes that were mid-episode drew again at step 26
    assert_league_equal(read_all(q), ref.state())
    assert_state_equal(b, o)
    b.close()


# ---- 5. frozen lanes ---------------------------------------------------------------------------------------------
def test_lanes_that_were_never_reset_contribute_nothing_and_keep_their_first_pick():
    K, n, player, off = 5, 67, 1, 6
    b, q = device(K, n, player, lane_offset=off, reset=False)
    q.run(3)
    r = read_all(q)
    assert b.misuse() == SoccerBatch.MISUSE_FROZEN and r["steps"] == 3
    assert (r["Q_a"][:, 1:] == 1.0).all() and (r["Q_b"][:, 1:] == 1.0).all() and (r["Q_a"][:, 0] == 0).all()
    assert (r["alpha"] == 1.0 * 0.99 * 0.99 * 0.99).all()
    T = league_thresholds(make_league(K, b.nS)[1])
    first = league_pick(T, lane_words(SEED, off + np.arange(n), 2 ** 62 + 0, purpose=1))     # the draw of the first run step, tick 0
    np.testing.assert_array_equal(r["pick"], first)
    o, ref = restatement(K, n, player, lane_offset=off)
    ref.run(o, np.zeros(n, np.uint16), 3)                       # no reset: every lane frozen
    assert ref.n_left_out == 3 * n and ref.n_redraws == 0
    assert_league_equal(r, ref.state())
    b.close()


# ---- 6. the Python surface ----------------------------------------------------------------------------------------
def test_vector_env_and_planner_entry_points_take_a_league():
    env = VectorSoccerEnv(67, 5, 4, 0.2, seed=SEED, autoreset=True)
    pol, w = make_league(5, env.nS)
    q = env.q_population(GAMMA, act_a="greedy", act_b="league", league_policies=pol, league_weights=w)
    env.reset(); q.run(10)
    picks = q.picks()
    assert q.league == 1 and picks.shape == (67,) and set(picks.tolist()) <= {-1, 1, 3}        # weights 0, 2 and 4 are zero
    e = q.exploitability(theta=1e-6, first=0, count=3)
    assert e["gap"].shape == (3, env.nS)
    q.close()
    out = pl.q_population(env, 20, GAMMA, act_a="league", act_b="greedy", league_policies=pol, league_weights=w, first=2, count=4)
    assert out[0].shape == (4, env.nS, 5) and (out[1].sum(2) == 1).all()
    env.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=True)
    nS = b.nS
    pol, w = make_league(3, nS)
    uni = np.full((nS, 5), 0.2)
    neg = np.array([0.5, -0.1, 0.6]); heavy = np.array([0.5, 0.25, 0.25 + 1.2e-5])
    off_row = pol.copy(); off_row[2, 7, 4] += 1.2e-5
    # the Python layer, as the class raises today: AssertionError before any library call
    for kw, msg in ((dict(league_policies=pol[:0], league_weights=w[:0]), "1 .. 1024 policies, not 0"),
                    (dict(league_policies=np.broadcast_to(uni, (1025, nS, 5)), league_weights=np.full(1025, 1.0 / 1025)), "1 .. 1024 policies, not 1025"),
                    (dict(league_policies=pol, league_weights=neg), r"league_weights\[1\] is negative"),
                    (dict(league_policies=pol, league_weights=heavy), "league_weights does not sum to 1"),
                    (dict(league_policies=off_row, league_weights=w), r"league_policies\[2\]\[7\]"),
                    (dict(league_policies=pol, league_weights=w[:2]), "one weight per league policy"),
                    (dict(), "league_policies")):
        with pytest.raises(AssertionError, match=msg):
            b.q_population(GAMMA, act_a="greedy", act_b="league", **kw)
    with pytest.raises(AssertionError, match="exactly one player may be a league"):
        b.q_population(GAMMA, act_a="league", act_b="league", league_policies=pol, league_weights=w)
    with pytest.raises(AssertionError, match="go with act_a or act_b = 'league'"):
        b.q_population(GAMMA, league_policies=pol, league_weights=w)
    # the library's own checks, straight through the ABI
    big = np.ascontiguousarray(np.broadcast_to(uni, (1025, nS, 5))); wbig = np.full(1025, 1.0 / 1025)
    F, G = _lib.QL_FIXED, _lib.QL_GREEDY

    def create(act_a, act_b, player, K, policies, weights, policy_a=None, policy_b=None):
        cfg = _lib.QPopulationConfig(0.9, 1.0, 0.5, 0.2, 1.0, act_a, act_b, policy_a, policy_b, None, None, None, None)
        out = C.c_void_p()
        code = b.lib.soccer_q_population_create_league(b.h, C.byref(cfg), player, K, policies.ctypes.data, weights.ctypes.data, C.byref(out))
        return code, out, b.lib.soccer_last_error(b.h).decode()
    for args, msg in (((G, F, 1, 0, pol, w), r"n_policies must be in 1 \.\. 1024, not 0"),
                      ((G, F, 1, 1025, big, wbig), r"n_policies must be in 1 \.\. 1024, not 1025"),
                      ((G, F, 1, 3, pol, neg), r"weights\[1\] is negative"),
                      ((G, F, 1, 3, pol, np.array([0.5, float("nan"), 0.5])), r"weights\[1\]"),
                      ((G, F, 1, 3, pol, heavy), "weights does not sum to 1"),
                      ((G, F, 1, 3, off_row, w), r"policies\[2\]\[7\] does not sum to 1"),
                      ((G, G, 1, 3, pol, w), "the league player must be SOCCER_QL_FIXED with a NULL policy"),
                      ((G, F, 1, 3, pol, w, None, uni.ctypes.data), "the league player must be SOCCER_QL_FIXED with a NULL policy"),
                      ((F, F, 1, 3, pol, w), "policy_a goes with act_a"),            # both players FIXED with NULL: one league only
                      ((G, F, 2, 3, pol, w), "league_player must be 0")):
        code, out, err = create(*args)
        assert code == _lib.E_INVALID and not out.value and re.search(msg, err), (msg, err)
    code, out, err = create(G, F, 1, 3, pol, np.array([0.5, 0.25, 0.25 + 9e-6]))       # inside the tolerance of a policy row
    assert code == _lib.OK and out.value and b.lib.soccer_q_population_destroy(b.h, out) == _lib.OK
    # the league calls on a population without one
    plain = b.q_population(GAMMA)
    with pytest.raises(AssertionError, match="has no league"):
        plain.picks()
    with pytest.raises(AssertionError, match="has no league"):
        plain.load_picks([0])
    # picks outside -1 .. K - 1, ranges outside the population; a refused load changes nothing
    q = b.q_population(GAMMA, act_a="league", act_b="greedy", league_policies=pol, league_weights=w)
    b.reset(); q.run(3)
    before = q.picks()
    assert (before >= 0).any()
    for bad, first, msg in (([0, 1, 3], 10, r"pick\[2\] = 3 is outside -1 \.\. 2"), ([-2], 0, r"pick\[0\] = -2"), ([0] * 5, 60, "outside the population")):
        with pytest.raises(AssertionError, match=msg):
            q.load_picks(bad, first=first)
        np.testing.assert_array_equal(q.picks(), before)
    with pytest.raises(AssertionError, match="outside the population"):
        q.picks(60, 5)
    b.graph_begin()
    b.rollout(2, sample_actions=True)           # (something to capture; never replayed)
    for call in (lambda: q.picks(), lambda: q.load_picks([0]),
                 lambda: b.q_population(GAMMA, act_a="league", league_policies=pol, league_weights=w)):
        with pytest.raises(RuntimeError, match="during graph capture"):
            call()
    b.graph_destroy(b.graph_end())
    b.close()
    assert q.q is None and plain.q is None
