"""-m gpu: the population of minimax-Q learners, a learner per lane (include/soccer_hip.h, "learners, a population of minimax-Q
learners") against its numpy restatement (tests/minimax_q_population_np.py: the oracle as environment, the host build of the
stage-game solver), bit for bit — update() on chosen transitions with near-tie games, run() from loaded states on seven shapes;
then launch boundaries and geometry, the defining test against a one-lane soccer_minimax_q learner, per-member
hyperparameters, round trips, frozen lanes, a shared handle, exploitability, the refusals, and the learning run."""
import ctypes as C
import os
import re
import sys
import time

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch, VectorSoccerEnv, _lib
from gym_soccer_littman94_amd import planners as pl
from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from minimax_q_population_np import ROWS, MinimaxQPopulationNumpy, assert_minimax_q_population_equal  # noqa: E402
from minimax_q_np import shapley_lists  # noqa: E402
from test_matrix_game_host import build_games_host, solve_host  # noqa: E402
from test_minimax_q_population_np import (BOUND, GAMMA, LEARN, N_UPDATE, RUN_CASES, RUN_IDS, RUN_KW, SEED, T_RUN, learning_grade,  # noqa: E402
                                          opponent_of, reference_run, update_case)

pytestmark = pytest.mark.gpu

DTYPES = (np.uint16, np.int8, np.int8, np.int8, np.uint8, np.uint16)
KEYS = ROWS + ("alpha",)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_games_host(tmp_path_factory.mktemp("games_gpu_mqpop"))


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


def assert_same_bits(got, want, keys=KEYS, where=""):
    for k in keys:
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (where, k)


# ---- 1. update() against numpy, exactly ---------------------------------------------------------------
def test_update_equals_numpy_bit_for_bit_and_leaves_bad_transitions_out(host):
    """67 members; members 30.. hold a near-tie game (DESIGN section 9's first hard family) at the state their transition hits,
    so the re-solve takes the enumeration fallback (tests/test_minimax_q_population_np.py counts it)"""
    ref, kw, start, batches, bad_act, bad_obs = update_case(host)
    n = N_UPDATE
    b = SoccerBatch(n, 5, 4, 0.0, seed=1, autoreset=True)
    q = b.minimax_q_population(GAMMA, **kw)
    fresh = MinimaxQPopulationNumpy(host, n, b.nS, GAMMA, **kw)
    assert_minimax_q_population_equal(q.read(), fresh.state())         # creation: set, not solved
    q.load(**start)                                                    # Q alone: every live state is re-solved on the device
    assert_minimax_q_population_equal(q.read(), ref.state())
    for batch, kp, flags in batches:
        before = q.read()
        q.update(*batch)
        ref.update(*batch, keep=kp)
        got = q.read()
        assert_minimax_q_population_equal(got, ref.state())
        assert b.misuse() == flags
        b.reset_stats()
        if kp is not None:
            for i in bad_act + bad_obs:             # flag raised, that member left alone, alpha advanced
                assert_same_bits({k: got[k][i] for k in ROWS}, {k: before[k][i] for k in ROWS}, ROWS, i)
                assert got["alpha"][i] == before["alpha"][i] * 0.9
        assert (got["Q"][:, 0] == 0).all() and (got["V"][:, 0] == 0).all()
    assert q.steps == 3 and (q.alpha == ref.alpha).all()
    assert ref.codes[0] > 0 and ref.codes[2] >= 1
    warm = batches[0][0]
    dev = [b.alloc(n, dt).upload(np.ascontiguousarray(x, dt)) for x, dt in zip(warm, DTYPES)]       # device arrays in
    q.update(*dev); ref.update(*warm)
    assert_minimax_q_population_equal(q.read(), ref.state())
    with pytest.raises(AssertionError, match="one transition per member"):
        q.update(*[x[:5] for x in warm])
    q.close(); b.close()


# ---- 2. run(T) from a loaded state against the restatement, exactly ------------------------------------------
def _device_run(host, parts, w=5, h=4, slip=0.2, opponent="self", n=67, max_steps=5, start=None, reset=True):
    """the device twin of reference_run: the same handle, the same loaded state, run(t) for t in parts"""
    if start is None:
        start = reference_run(host, w, h, slip, opponent, n, max_steps)[2]
    b = SoccerBatch(n, w, h, slip, seed=SEED, autoreset=True, max_steps=max_steps)
    q = b.minimax_q_population(GAMMA, opponent=opponent_of(opponent, n, b.nS), **RUN_KW)
    q.load(**start)
    if reset:
        b.reset()
    for t in parts:
        q.run(t)
    return b, q


@pytest.mark.parametrize("case", RUN_CASES, ids=RUN_IDS)
def test_run_equals_the_restatement_bit_for_bit(host, case):
    """run() caps its grid at 8 192 waves on this device, above every member count used here: a wave per
    member.  test_result_does_not_depend_on_the_waves_of_a_launch lowers the cap, so that there are more members than waves."""
    w, h, slip, opponent, n, max_steps = case
    o, ref, start = reference_run(host, w, h, slip, opponent, n, max_steps)
    b, q = _device_run(host, [T_RUN], w, h, slip, opponent, n, max_steps)
    assert_minimax_q_population_equal(q.read(), ref.state())
    assert_state_equal(b, o)
    assert b.tick == o.tick == T_RUN + 1
    hist, misuse = b.stats()
    np.testing.assert_array_equal(hist, o.hist)
    assert misuse == 0 and ref.n_left_out == 0
    assert ref.codes[0] > 0                                            # mixed games were solved by the simplex path
    assert q.steps == T_RUN and (q.alpha == ref.alpha).all()
    part = q.read(n // 2, 1)                       # a range is the slice
    assert part["pi_b"].tobytes() == ref.pi_b[n // 2:n // 2 + 1].tobytes() and part["alpha"][0] == ref.alpha[n // 2]
    b.close()


# ---- 3. launch boundaries, invariance --------------------------------------------------------------------
def test_runs_compose(host):
    b1, q1 = _device_run(host, [60]); b2, q2 = _device_run(host, [25, 35])
    assert_minimax_q_population_equal(q2.read(), q1.read())
    assert_batches_equal(b1, b2)
    assert_minimax_q_population_equal(q1.read(), reference_run(host, 5, 4, 0.2, "self", 67, 5)[1].state())
    b1.close(); b2.close()


def test_result_does_not_depend_on_the_steps_per_launch(host, monkeypatch):
    """slip 0: a Philox block spans eight ticks, so with seven steps per launch a launch starts in the middle of a block"""
    args = dict(slip=0.0, opponent="uniform", n=259, max_steps=100)
    b1, q1 = _device_run(host, [60], **args)
    monkeypatch.setenv("SOCCER_POP_LAUNCH_STEPS", "7")
    b2, q2 = _device_run(host, [60], **args)
    monkeypatch.delenv("SOCCER_POP_LAUNCH_STEPS")
    assert_minimax_q_population_equal(q2.read(), q1.read())
    assert_batches_equal(b1, b2)
    assert_minimax_q_population_equal(q1.read(), reference_run(host, 5, 4, 0.0, "uniform", 259)[1].state())
    b1.close(); b2.close()


def test_result_does_not_depend_on_the_waves_of_a_launch(host, monkeypatch):
    """259 members on 100 waves (SOCCER_MQ_POP_WAVES, read at creation): a wave serves two or three members in turn, the
    last round of the member loop is ragged; load()'s re-solve and update() go through the same grid"""
    args = dict(slip=0.2, opponent="dirichlet", n=259, max_steps=5)
    monkeypatch.setenv("SOCCER_MQ_POP_WAVES", "100")
    b, q = _device_run(host, [25, 35], **args)
    monkeypatch.delenv("SOCCER_MQ_POP_WAVES")
    o, ref, _ = reference_run(host, 5, 4, 0.2, "dirichlet", 259, 5)
    assert_minimax_q_population_equal(q.read(), ref.state())
    assert_state_equal(b, o)
    np.testing.assert_array_equal(b.stats()[0], o.hist)
    b.close()


def test_result_does_not_depend_on_the_state_layout(host, monkeypatch):
    b1, q1 = _device_run(host, [40])
    monkeypatch.setenv("SOCCER_STATE_LAYOUT", "wide")
    b2, q2 = _device_run(host, [40])
    monkeypatch.delenv("SOCCER_STATE_LAYOUT")
    assert b1.state_streams() == 3 and b2.state_streams() == 6
    assert_minimax_q_population_equal(q2.read(), q1.read())
    assert_batches_equal(b1, b2)
    b1.close(); b2.close()


# ---- 4. the defining test ---------------------------------------------------------------------------------
@pytest.mark.parametrize("opponent", ["uniform", "self", "fixed"])
def test_a_population_of_one_is_the_shared_learner_with_one_lane(host, opponent):
    """a one-member population equals a soccer_minimax_q learner on a one-lane handle with the same seed over 60 steps, bit for
    bit, from a fresh table (strategies set, not solved) and from a loaded random table (both re-solve every state)"""
    T = 60
    for seed, loaded in ((3, False), (4, True)):
        b1 = SoccerBatch(1, 5, 4, 0.2, seed=seed, autoreset=True, max_steps=5)
        b2 = SoccerBatch(1, 5, 4, 0.2, seed=seed, autoreset=True, max_steps=5)
        opp = opponent_of(opponent, 1, b1.nS)
        kw = dict(alpha=0.9, decay=0.98, explor=0.3, q_init=0.25)
        q1 = b1.minimax_q_population(GAMMA, opponent=opp, **kw)
        q2 = b2.minimax_q(GAMMA, opponent=opp, **kw)
        if loaded:
            Q = np.zeros((b1.nS, 5, 5)); Q[1:] = np.random.default_rng(seed).uniform(-1.0, 1.0, (b1.nS - 1, 5, 5))
            q1.load(Q=Q[None]); q2.load(Q)
        b1.reset(); b2.reset()
        q1.run(T); q2.run(T)
        r1, r2 = q1.read(), q2.read()
        for k in ROWS:
            assert r1[k][0].tobytes() == r2[k].tobytes(), (opponent, loaded, k)
        assert r1["alpha"][0] == r2["alpha"] and r1["steps"] == r2["steps"] == T
        assert int(r2["visits"].sum()) == T and (r1["pi_a"][0] != 0.2).any()
        assert_batches_equal(b1, b2)
        b1.close(); b2.close()


# ---- 5. per-member hyperparameters ---------------------------------------------------------------------
def test_per_member_hyperparameters(host):
    """per-member arrays for all four hyperparameters: every member against the restatement, and a SAMPLE of the members (every
    eleventh and the last, 8 of 67) against a population created with that member's values as scalars"""
    n = 67
    rng = np.random.default_rng(3)
    HYPER = dict(alpha=rng.uniform(0.2, 1.0, n), decay=rng.uniform(0.9, 1.0, n), explor=rng.uniform(0.0, 1.0, n))
    gam = rng.uniform(0.0, 0.99, n)
    o = Oracle(5, 4, 0.2, n=n, seed=SEED, autoreset=True)
    ref = MinimaxQPopulationNumpy(host, n, o.nS, gam, opponent="self", **HYPER)
    start = ref.load(np.random.default_rng(4))
    ref.run(o, o.reset(), T_RUN)
    b = SoccerBatch(n, 5, 4, 0.2, seed=SEED, autoreset=True)
    q = b.minimax_q_population(gam, opponent="self", **HYPER)
    q.load(**start)
    b.reset(); q.run(T_RUN)
    got = q.read()
    assert_minimax_q_population_equal(got, ref.state())
    assert_state_equal(b, o)
    np.testing.assert_array_equal(q.discount_factor, gam)
    b.close()
    # member i alone: a population created with i's values as scalars has the same member i while i's lane sees the same
    # actions — its own — so from the same loaded state it is member i of the run above
    for i in list(range(0, n, 11)) + [n - 1]:
        b1 = SoccerBatch(n, 5, 4, 0.2, seed=SEED, autoreset=True)
        q1 = b1.minimax_q_population(float(gam[i]), opponent="self", **{k: float(v[i]) for k, v in HYPER.items()})
        q1.load(**start)
        b1.reset(); q1.run(T_RUN)
        one = q1.read(i, 1)
        assert_same_bits({k: one[k][0] for k in KEYS}, {k: got[k][i] for k in KEYS}, where=i)
        b1.close()


# ---- 6. round trips, frozen lanes --------------------------------------------------------------------------
def test_read_then_load_of_a_range_on_a_fresh_population_continues_the_same(host):
    """from a FRESH table, so that most states have never been updated when the checkpoint is taken: their strategies are the
    0.2 rows creation set, which no solve of Q would give back"""
    first, count, n = 10, 30, 67
    kw = dict(RUN_KW, q_init=0.25)

    def fresh_run(parts):
        b = SoccerBatch(n, 5, 4, 0.2, seed=SEED, autoreset=True, max_steps=5)
        q = b.minimax_q_population(GAMMA, opponent="self", **kw)
        b.reset()
        for t in parts:
            q.run(t)
        return b, q
    b1, q1 = fresh_run([60])
    b2, q2 = fresh_run([25])
    ck = q2.read(first, count)
    never = (ck["pi_a"] == 0.2).all(2)
    assert never[:, 1:].any() and not never[:, 1:].all()               # states never visited, and states solved
    q3 = b2.minimax_q_population(GAMMA, opponent="self", **kw)         # a second, fresh population on the same handle
    fresh = q3.read()
    q3.load(**{k: ck[k] for k in KEYS + ("steps",)}, first=first)
    now = q3.read()
    assert_minimax_q_population_equal(q3.read(first, count), ck)
    for k in KEYS:                                                     # nothing outside the range moved
        assert now[k][:first].tobytes() == fresh[k][:first].tobytes() and now[k][first + count:].tobytes() == fresh[k][first + count:].tobytes()
    q3.run(35)
    assert_minimax_q_population_equal(q3.read(first, count), q1.read(first, count))
    # one array alone: the others stay, nothing is solved
    q3.load(pi_b=ck["pi_b"], first=first)
    r = q3.read(first, count)
    assert r["pi_b"].tobytes() == ck["pi_b"].tobytes()
    assert_same_bits(r, q1.read(first, count), [k for k in KEYS if k != "pi_b"])
    q3.load(V=ck["V"], first=first)
    r = q3.read(first, count)
    assert r["V"].tobytes() == ck["V"].tobytes() and r["pi_a"].tobytes() == q1.read(first, count)["pi_a"].tobytes()
    # Q alone: every live state of the range is re-solved — solve_host's bits — and nothing outside it
    before = q3.read()
    Q = np.zeros((count, b2.nS, 5, 5)); Q[:, 1:] = np.random.default_rng(6).uniform(-1.0, 1.0, (count, b2.nS - 1, 5, 5))
    Q[:, 0] = 7.0                                                      # row 0 is taken as zeros
    q3.load(Q=Q, first=first)
    r = q3.read()
    v, x, y, code = solve_host(host, Q[:, 1:].reshape(-1, 5, 5))
    assert (code == 0).any()
    sl = slice(first, first + count)
    assert r["Q"][sl, 1:].tobytes() == Q[:, 1:].tobytes() and (r["Q"][sl, 0] == 0).all() and (r["V"][sl, 0] == 0).all()
    assert r["V"][sl, 1:].tobytes() == v.tobytes() and r["pi_a"][sl, 1:].tobytes() == x.tobytes() and r["pi_b"][sl, 1:].tobytes() == y.tobytes()
    assert (r["pi_a"][sl, 0] == 0.2).all()
    for k in KEYS:
        assert r[k][:first].tobytes() == before[k][:first].tobytes() and r[k][first + count:].tobytes() == before[k][first + count:].tobytes()
    # a refused load changes nothing (the Python layer checks first, so straight through the ABI)
    before = q3.read()
    nS = b2.nS
    bad_q = ck["Q"].copy(); bad_q[count - 1, nS - 1, 4, 3] = 1.5
    bad_v = ck["V"].copy(); bad_v[2, 5] = -1.25
    bad_pi = ck["pi_a"].copy(); bad_pi[7, 3] = [0.5, 0.5, 0.5, 0.0, 0.0]
    bad_pb = ck["pi_b"].copy(); bad_pb[8, 9, 2] = -0.25
    bad_al = ck["alpha"].copy(); bad_al[-1] = 2.0

    def ptrs(**kw):
        return [kw[k].ctypes.data if k in kw else None for k in KEYS] + [None]
    for (f, c, args), msg in (((first, count, ptrs(Q=bad_q, V=ck["V"])), r"Q\[29\]\[%d\]\[4\]\[3\] is outside" % (nS - 1)),
                              ((first, count, ptrs(Q=ck["Q"], V=bad_v)), r"V\[2\]\[5\] is outside"),
                              ((first, count, ptrs(Q=ck["Q"], pi_a=bad_pi)), r"pi_a\[7\]\[3\] does not sum to 1"),
                              ((first, count, ptrs(Q=ck["Q"], pi_b=bad_pb)), r"pi_b\[8\]\[9\]\[2\] is negative"),
                              ((first, count, ptrs(Q=ck["Q"], alpha=bad_al)), r"alpha\[29\]"),
                              ((60, 10, ptrs(Q=ck["Q"])), "outside the population"),
                              ((-1, 1, ptrs()), "outside the population")):
        assert b2.lib.soccer_minimax_q_population_load(b2.h, q3.q, f, c, *args) == _lib.E_INVALID
        assert re.search(msg, b2.lib.soccer_last_error(b2.h).decode()), (msg, b2.lib.soccer_last_error(b2.h))
        assert_minimax_q_population_equal(q3.read(), before)
    with pytest.raises(AssertionError, match="\\[-1, 1\\]"):
        q3.load(bad_q, first=first)
    b1.close(); b2.close()
    assert q3.q is None and q2.q is None                               # the handle freed both


def test_lanes_that_were_never_reset_contribute_nothing():
    n = 67
    b = SoccerBatch(n, 5, 4, 0.2, seed=SEED, autoreset=True)
    q = b.minimax_q_population(GAMMA, alpha=0.8, decay=0.5, q_init=0.25)
    q.run(3)
    r = q.read()
    assert b.misuse() == SoccerBatch.MISUSE_FROZEN and r["steps"] == 3
    assert (r["Q"][:, 1:] == 0.25).all() and (r["V"][:, 1:] == 0.25).all() and (r["Q"][:, 0] == 0).all() and (r["V"][:, 0] == 0).all()
    assert (r["pi_a"] == 0.2).all() and (r["pi_b"] == 0.2).all()
    assert (r["alpha"] == 0.8 * 0.5 * 0.5 * 0.5).all()
    b.close()


# ---- 7. a shared handle, exploitability ---------------------------------------------------------------------
def test_a_population_a_q_population_and_a_shared_learner_share_a_handle():
    """a minimax-Q population, a Q-population and a shared-table minimax-Q learner alive on one handle, run one after the other
    from the same checkpoint (state and tick): each equals its run alone"""
    T, n = 20, 259
    kw = dict(explor=0.2, decay=0.99)

    def make(b):
        return (b.minimax_q_population(GAMMA, opponent="self", **kw), b.q_population(GAMMA, **kw), b.minimax_q(GAMMA, opponent="self", **kw))
    b = SoccerBatch(n, 5, 4, 0.2, seed=SEED, autoreset=True)
    shared = make(b)
    b.reset()
    ck = b.checkpoint()
    for q in shared:
        b.restore(ck)
        q.run(T)
    for i in range(3):
        b1 = SoccerBatch(n, 5, 4, 0.2, seed=SEED, autoreset=True)
        alone = make(b1)[i]
        b1.reset(); alone.run(T)
        got, want = shared[i].read(), alone.read()
        assert sorted(got) == sorted(want)
        for k in got:
            assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (i, k)
        assert b.tick == b1.tick == T + 1
        b1.close()
    b.close()
    assert all(q.q is None for q in shared)                    # the handle freed all three


def test_exploitability_of_300_members_is_each_member_s_own(host):
    n = 300
    b = SoccerBatch(n, 5, 4, 0.0, seed=SEED, autoreset=True)
    q = b.minimax_q_population(GAMMA, opponent="self", **RUN_KW)
    Q = np.zeros((n, b.nS, 5, 5)); Q[:, 1:] = np.random.default_rng(9).uniform(-1.0, 1.0, (n, b.nS - 1, 5, 5))
    q.load(Q=Q)
    b.reset(); q.run(30)
    r = q.read()
    e = q.exploitability(theta=1e-6)
    assert e["gap"].shape == e["v_a"].shape == e["v_b"].shape == (n, b.nS)
    for i in (0, 1, 137, 255, 256, 299):                # both chunks and their boundary
        one = pl.exploitability(b, r["pi_a"][i], r["pi_b"][i], 1e-6, GAMMA)
        for k in ("v_a", "v_b", "gap"):
            assert e[k][i].tobytes() == one[k].tobytes(), (i, k)
    assert (e["gap"][:, 1:] >= -1e-4).all()          # theta / (1 - gamma), with room
    part = q.exploitability(theta=1e-6, first=250, count=7)
    assert part["gap"].tobytes() == e["gap"][250:257].tobytes()
    b.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=False)
    with pytest.raises(AssertionError, match="SOCCER_F_AUTORESET"):
        b.minimax_q_population(GAMMA)
    b.close()
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=True)
    b.set_policy("player_b", np.zeros(b.nS, np.int8))
    with pytest.raises(AssertionError, match="two-player handle"):
        b.minimax_q_population(GAMMA)
    b.set_policy("player_b", None)
    q = b.minimax_q_population(GAMMA)
    with pytest.raises(AssertionError, match="outside the population"):
        q.read(60, 5)
    for first, count in ((65, 0), (0, 65), (-1, 2), (3, -1), (2 ** 62, 2 ** 62)):
        assert b.lib.soccer_minimax_q_population_read(b.h, q.q, first, count, None, None, None, None, None, None) == _lib.E_INVALID
        assert "outside the population" in b.lib.soccer_last_error(b.h).decode()
    dev = [b.alloc(64, dt).fill(0) for dt in DTYPES]
    b.sync()
    b.graph_begin()
    b.rollout(2, sample_actions=True)           # (something to capture; never replayed)
    for call in (lambda: q.run(1), lambda: q.read(), lambda: q.load(np.zeros((64, b.nS, 5, 5))), lambda: b.minimax_q_population(GAMMA),
                 lambda: q.update(*dev), lambda: q.steps, lambda: q.alpha):
        with pytest.raises(RuntimeError, match="during graph capture"):
            call()
    b.graph_destroy(b.graph_end())
    other = SoccerBatch(64, 5, 4, 0.0, autoreset=True)
    with pytest.raises(AssertionError, match="not a population of this handle"):
        other._check(other.lib.soccer_minimax_q_population_run(other.h, q.q, 1))
    other.close()
    with pytest.raises(AssertionError, match="n_steps must be >= 0"):
        q.run(-1)
    assert b.lib.soccer_minimax_q_population_update(b.h, q.q, dev[0].ptr, None, None, None, None, None) == _lib.E_INVALID
    assert "all six transition arrays" in b.lib.soccer_last_error(b.h).decode()
    # the library's own range checks (the Python layer checks first, so straight through the ABI)
    uniform = np.full((b.nS, 5), 0.2)
    bad_row = uniform.copy(); bad_row[3] = [0.5, 0.5, 0.5, 0.0, 0.0]
    ok_each = np.full((64, b.nS, 5), 0.2)
    bad_each = ok_each.copy(); bad_each[41, 17, 2] = float("nan")
    ok64 = np.full(64, 0.5)

    def arr(i, v):
        a = ok64.copy(); a[i] = v
        return a
    keep = [arr(7, 1.0), arr(8, -0.5), arr(9, 0.0), arr(63, 2.0)]
    FIELDS = [f for f, _ in _lib.MinimaxQPopulationConfig._fields_]
    for fields, msg in ((dict(discount_factor=1.0), "discount_factor"), (dict(alpha=-0.5), "alpha"), (dict(decay=0.0), "decay"),
                        (dict(explor=2.0), "explor"), (dict(q_init=-1.5), "q_init"), (dict(opponent=7), "opponent must be"),
                        (dict(opponent=_lib.MQ_FIXED), "exactly one of opponent_policy and opponent_policy_per_member"),
                        (dict(opponent_policy=uniform.ctypes.data), "exactly one of opponent_policy and opponent_policy_per_member"),
                        (dict(opponent=_lib.MQ_SELF, opponent_policy_per_member=ok_each.ctypes.data), "exactly one of opponent_policy"),
                        (dict(opponent=_lib.MQ_FIXED, opponent_policy=uniform.ctypes.data, opponent_policy_per_member=ok_each.ctypes.data),
                         "exactly one of opponent_policy"),
                        (dict(opponent=_lib.MQ_FIXED, opponent_policy=bad_row.ctypes.data), "opponent_policy\\[0\\]\\[3\\] does not sum to 1"),
                        (dict(opponent=_lib.MQ_FIXED, opponent_policy_per_member=bad_each.ctypes.data),
                         "opponent_policy_per_member\\[41\\]\\[17\\]\\[2\\] is negative or not a number"),
                        (dict(discount_factor_per_member=keep[0].ctypes.data), "discount_factor_per_member\\[7\\]"),
                        (dict(alpha_per_member=keep[1].ctypes.data), "alpha_per_member\\[8\\]"),
                        (dict(decay_per_member=keep[2].ctypes.data), "decay_per_member\\[9\\]"),
                        (dict(explor_per_member=keep[3].ctypes.data), "explor_per_member\\[63\\]")):
        cfg = _lib.MinimaxQPopulationConfig(0.9, 1.0, 0.5, 0.2, 1.0, 0, 0)
        for k, v in fields.items():
            assert k in FIELDS
            setattr(cfg, k, v)
        out = C.c_void_p()
        assert b.lib.soccer_minimax_q_population_create(b.h, C.byref(cfg), C.byref(out)) == _lib.E_INVALID and not out.value
        assert re.search(msg, b.lib.soccer_last_error(b.h).decode()), (msg, b.lib.soccer_last_error(b.h))
    # a per-member array overrides a scalar that is out of range: only what is used is checked
    cfg = _lib.MinimaxQPopulationConfig(0.9, 7.0, 0.5, 0.2, 1.0, 0, 0)
    cfg.alpha_per_member = ok64.ctypes.data
    out = C.c_void_p()
    assert b.lib.soccer_minimax_q_population_create(b.h, C.byref(cfg), C.byref(out)) == _lib.OK and out.value
    assert b.lib.soccer_minimax_q_population_destroy(b.h, out) == _lib.OK
    fixed = b.minimax_q_population(GAMMA, opponent=uniform)
    b.reset(); q.run(2); fixed.run(2)
    assert q.steps == 2 and fixed.steps == 2 and b.tick == 5 and b.misuse() == 0
    b.close()                                   # with live populations: the handle frees them
    assert fixed.q is None and q.q is None
    q.close()                                   # the wrapper knows


# ---- 9. it learns -----------------------------------------------------------------------------------------
def test_every_member_learns_who_scores_where(host):
    """The learning run of tests/test_minimax_q_population_np.py on the device, same n, T and seed, so the restatement's figures
    are the device's (test 2 pins the bits): Littman's MR, 64 one-actor learners from Q = 0, alpha 1 -> 0.01.  Asserted: the
    population mean of the share of the scoring cells where Q_i lacks the reward's sign stays under BOUND (untrained: 1.0), and
    both V figures improve.  Printed beside it: mean |V_i - V*| over the decided states and over all live states, whose
    doubled worst cases do not lie below their untrained figures at this budget."""
    c = LEARN
    lists = shapley_lists(Oracle(c["width"], c["height"], c["slip"], n=4, seed=c["seed"], autoreset=True))
    env = VectorSoccerEnv(c["n"], c["width"], c["height"], c["slip"], seed=c["seed"], autoreset=True)
    vstar = pl.minimax_value_iteration(env, 1e-10, c["gamma"])[2]
    q = env.minimax_q_population(c["gamma"], alpha=c["alpha"], decay=0.01 ** (1.0 / c["T"]), explor=c["explor"], q_init=c["q_init"],
                                 opponent="uniform")
    env.reset()
    env._batch.sync()
    t0 = time.perf_counter()
    q.run(c["T"])
    steps = q.steps                             # synchronises
    wall = time.perf_counter() - t0
    r = q.read()
    share, err, untrained, err_all, untrained_all = learning_grade(r["Q"], r["V"], lists, vstar)
    print("MR, %d members x %d steps: scoring cells without the reward's sign, population mean %.6f (members %.6f .. %.6f), untrained 1.0; "
          "decided states %.6f (%.6f .. %.6f), untrained %.6f; all live states %.6f (%.6f .. %.6f), untrained %.6f; run() took %.3f s = "
          "%.2f us per step" % (c["n"], c["T"], share.mean(), share.min(), share.max(), err.mean(), err.min(), err.max(), untrained,
                                err_all.mean(), err_all.min(), err_all.max(), untrained_all, wall, wall / c["T"] * 1e6))
    assert steps == c["T"] and np.abs(r["alpha"] - 0.01).max() < 1e-9
    assert (r["pi_b"][:, 0] == 0.2).all() and np.abs(r["pi_a"].sum(2) - 1.0).max() < 1e-12
    assert share.mean() <= BOUND
    assert err_all.mean() < untrained_all and err.mean() < untrained
    out = pl.minimax_q_population(env, 50, c["gamma"], q_init=0.0, opponent="self", first=3, count=5)      # the planner-style entry point
    assert all(x.shape == (5, env.nS, 5) for x in out[:2]) and out[2].shape == (5, env.nS) and out[3].shape == (5, env.nS, 5, 5) and out[4].shape == (5,)
    assert np.abs(out[0][:, 1:].sum(2) - 1.0).max() < 1e-12
    q.close(); env.close()
