"""-m gpu: the population of policy hill-climbers, a PHC / WoLF-PHC learner per lane (include/soccer_hip.h, "learners, a
population of policy hill-climbers") against its numpy restatement (tests/wolf_population_np.py: the oracle as environment),
bit for bit — update() on chosen transitions, run() from loaded states on six shapes; then launch boundaries, per-member
hyperparameters, invariance and round trips, frozen lanes, the fixed policies (adopt, host path, shared), the Q side against
a QPopulation, a shared handle, exploitability, the refusals, and the learning run against the exact best response."""
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
from wolf_population_np import ROWS, WolfPopulationNumpy, assert_wolf_population_equal  # noqa: E402
from test_wolf_population_np import BOUND, GAMMA, LEARN, RUN_CASES, RUN_IDS, RUN_KW, SEED, T_RUN, act, reference_run  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = (np.uint16, np.int8, np.int8, np.int8, np.uint8, np.uint16)
KEYS = ROWS + ("updates", "alpha", "dscale")


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
def _valid(rng, nS, n):
    """obs, act_a, act_b, reward, terminated, next_obs; a reward is non-zero only on a terminated transition"""
    obs = rng.integers(1, nS, n); term = rng.random(n) < 0.3
    nxt = np.where(term, 0, rng.integers(0, nS, n))
    rew = np.where(term, rng.choice([-1, 1], n), 0)
    return [obs, rng.integers(0, 5, n), rng.integers(0, 5, n), rew, term.astype(np.uint8), nxt]


def test_update_equals_numpy_bit_for_bit_and_leaves_bad_transitions_out():
    n = 67
    b = SoccerBatch(n, 5, 4, 0.0, seed=1, autoreset=True)
    nS = b.nS
    kw = dict(alpha=0.75, decay=0.9, explor=0.2, q_init=0.5, delta_win=0.1, delta_lose=0.4, delta_decay=0.8)
    q = b.wolf_population(GAMMA, **kw)
    ref = WolfPopulationNumpy(n, nS, GAMMA, **kw)
    assert_wolf_population_equal(q.read(), ref.state())
    q.load(**ref.load(np.random.default_rng(2)))
    assert_wolf_population_equal(q.read(), ref.state())
    rng = np.random.default_rng(1994)
    warm = _valid(rng, nS, n)
    case = _valid(rng, nS, n)

    def put(i, s, a, bb, r, term, s2):
        for k, v in enumerate((s, a, bb, r, term, s2)):
            case[k][i] = v
    put(0, 17, 2, 0, 0, 0, 17)          # s' == s: the bootstrap is the row before the update
    put(1, 5, 0, 4, 1, 1, 0)            # terminated, next_obs 0, r = +1
    put(2, 5, 4, 4, -1, 1, 0)           # r = -1
    put(4, 17, 1, 1, 1, 1, 300)         # terminated with a live next_obs: still no bootstrap
    bad_act, bad_obs = [10, 11, 12], [20, 21, 22]
    case[1][10] = 5; case[2][11] = -1; case[1][12] = 100
    case[0][20] = 0; case[0][21] = nS; case[5][22] = nS + 3
    keep = np.ones(n, bool); keep[bad_act + bad_obs] = False
    for batch, kp, flags in ((warm, None, 0), (case, keep, SoccerBatch.MISUSE_ACTION | SoccerBatch.MISUSE_OBSERVATION), (warm, None, 0)):
        before = q.read()
        q.update(*batch)
        ref.update(*batch, keep=kp)
        got = q.read()
        assert_wolf_population_equal(got, ref.state())
        assert b.misuse() == flags
        b.reset_stats()
        if kp is not None:
            for i in bad_act + bad_obs:             # flag raised, that member's rows unchanged, alpha and dscale advanced
                assert_same_bits({k: got[k][i] for k in ROWS + ("updates",)}, {k: before[k][i] for k in ROWS + ("updates",)}, ROWS + ("updates",), i)
                assert got["alpha"][i] == before["alpha"][i] * 0.9 and got["dscale"][i] == before["dscale"][i] * 0.8
        assert ((got["updates"] != before["updates"]).sum(1) <= 1).all() and (got["Q_a"][:, 0] == 0).all() and (got["Q_b"][:, 0] == 0).all()
    assert q.steps == 3 and (q.alpha == ref.alpha).all() and (q.dscale == ref.dscale).all()
    assert ref.n_win > 0 and ref.n_lose > 0 and ref.n_clamp > 0
    dev = [b.alloc(n, dt).upload(np.ascontiguousarray(x, dt)) for x, dt in zip(warm, DTYPES)]       # device arrays in
    q.update(*dev); ref.update(*warm)
    assert_wolf_population_equal(q.read(), ref.state())
    with pytest.raises(AssertionError, match="one transition per member"):
        q.update(*[x[:5] for x in warm])
    q.close(); b.close()


# ---- 2. run(T) from a loaded state against the restatement, exactly ------------------------------------------
def _device_run(parts, w=5, h=4, slip=0.2, act_a="learn", act_b="learn", n=259, max_steps=6, extra=(), start=None, reset=True):
    """the device twin of reference_run: the same handle, the same loaded state, run(t) for t in parts"""
    if start is None:
        start = reference_run(w, h, slip, act_a, act_b, n, max_steps, extra)[2]
    b = SoccerBatch(n, w, h, slip, seed=SEED, autoreset=True, max_steps=max_steps)
    kw = dict(RUN_KW); kw.update(dict(extra))
    q = b.wolf_population(GAMMA, act_a=act(act_a, n, b.nS), act_b=act(act_b, n, b.nS), **kw)
    q.load(**start)
    if reset:
        b.reset()
    for t in parts:
        q.run(t)
    return b, q


@pytest.mark.parametrize("case", RUN_CASES, ids=RUN_IDS)
def test_run_equals_the_restatement_bit_for_bit(case):
    w, h, slip, act_a, act_b, n, max_steps, extra = case
    o, ref, start = reference_run(w, h, slip, act_a, act_b, n, max_steps, extra)
    b, q = _device_run([T_RUN], w, h, slip, act_a, act_b, n, max_steps, extra)
    assert_wolf_population_equal(q.read(), ref.state())
    assert_state_equal(b, o)
    assert b.tick == o.tick == T_RUN + 1
    hist, misuse = b.stats()
    np.testing.assert_array_equal(hist, o.hist)
    assert misuse == 0 and ref.n_left_out == 0
    assert ref.n_win > 0 and ref.n_lose > 0 and ref.n_clamp > 0            # every branch of the policy step was taken
    assert q.steps == T_RUN and (q.alpha == ref.alpha).all() and (q.dscale == ref.dscale).all()
    part = q.read(n // 2, 1)                       # a range is the slice
    assert part["pi_b"].tobytes() == ref.pi[1][n // 2:n // 2 + 1].tobytes() and part["alpha"][0] == ref.alpha[n // 2]
    b.close()


# ---- 3. launch boundaries, invariance --------------------------------------------------------------------
def test_runs_compose():
    b1, q1 = _device_run([60]); b2, q2 = _device_run([25, 35])
    assert_wolf_population_equal(q2.read(), q1.read())
    assert_batches_equal(b1, b2)
    assert_wolf_population_equal(q1.read(), reference_run(5, 4, 0.2, "learn", "learn", 259, 6)[1].state())
    b1.close(); b2.close()


def test_result_does_not_depend_on_the_steps_per_launch(monkeypatch):
    """slip 0: a Philox block spans eight ticks, so with seven steps per launch a launch starts in the middle of a block"""
    args = dict(slip=0.0, act_b="uniform", n=67, max_steps=100)
    b1, q1 = _device_run([60], **args)
    monkeypatch.setenv("SOCCER_POP_LAUNCH_STEPS", "7")
    b2, q2 = _device_run([60], **args)
    monkeypatch.delenv("SOCCER_POP_LAUNCH_STEPS")
    assert_wolf_population_equal(q2.read(), q1.read())
    assert_batches_equal(b1, b2)
    assert_wolf_population_equal(q1.read(), reference_run(5, 4, 0.0, "learn", "uniform", 67)[1].state())
    b1.close(); b2.close()


def test_result_does_not_depend_on_the_state_layout(monkeypatch):
    b1, q1 = _device_run([40])
    monkeypatch.setenv("SOCCER_STATE_LAYOUT", "wide")
    b2, q2 = _device_run([40])
    monkeypatch.delenv("SOCCER_STATE_LAYOUT")
    assert b1.state_streams() == 3 and b2.state_streams() == 6
    assert_wolf_population_equal(q2.read(), q1.read())
    assert_batches_equal(b1, b2)
    b1.close(); b2.close()


# ---- 4. per-member hyperparameters ---------------------------------------------------------------------
def test_per_member_hyperparameters():
    n = 67
    rng = np.random.default_rng(3)
    HYPER = dict(alpha=rng.uniform(0.2, 1.0, n), decay=rng.uniform(0.9, 1.0, n), explor=rng.uniform(0.0, 1.0, n),
                 delta_win=rng.uniform(0.0, 0.2, n), delta_lose=rng.uniform(0.2, 1.0, n), delta_decay=rng.uniform(0.95, 1.0, n))
    gam = rng.uniform(0.0, 0.99, n)
    o = Oracle(5, 4, 0.2, n=n, seed=SEED, autoreset=True)
    ref = WolfPopulationNumpy(n, o.nS, gam, **HYPER)
    start = ref.load(np.random.default_rng(4))
    ref.run(o, o.reset(), T_RUN)
    b = SoccerBatch(n, 5, 4, 0.2, seed=SEED, autoreset=True)
    q = b.wolf_population(gam, **HYPER)
    q.load(**start)
    b.reset(); q.run(T_RUN)
    got = q.read()
    assert_wolf_population_equal(got, ref.state())
    assert_state_equal(b, o)
    np.testing.assert_array_equal(q.discount_factor, gam)
    assert ref.n_win > 0 and ref.n_lose > 0 and ref.n_clamp > 0
    b.close()
    # member i alone: a population created with i's values as scalars has the same member i while i's lane sees the same
    # actions — its own — so from the same loaded state it is member i of the run above
    for i in list(range(0, n, 11)) + [n - 1]:
        b1 = SoccerBatch(n, 5, 4, 0.2, seed=SEED, autoreset=True)
        q1 = b1.wolf_population(float(gam[i]), **{k: float(v[i]) for k, v in HYPER.items()})
        q1.load(**start)
        b1.reset(); q1.run(T_RUN)
        one = q1.read(i, 1)
        assert_same_bits({k: one[k][0] for k in KEYS}, {k: got[k][i] for k in KEYS}, where=i)
        b1.close()


# ---- 5. round trips, frozen lanes --------------------------------------------------------------------------
def test_read_then_load_of_a_range_on_a_fresh_population_continues_the_same():
    first, count = 10, 30
    extra = {"delta_decay": 0.98}
    b1, q1 = _device_run([60], extra=extra)
    b2, q2 = _device_run([25], extra=extra)
    ck = q2.read(first, count)
    kw = dict(RUN_KW); kw.update(extra)
    q3 = b2.wolf_population(GAMMA, **kw)                               # a second, fresh population on the same handle
    fresh = q3.read()
    q3.load(**{k: ck[k] for k in KEYS + ("steps",)}, first=first)
    now = q3.read()
    assert_wolf_population_equal(q3.read(first, count), ck)
    for k in KEYS:                                                     # nothing outside the range moved
        assert now[k][:first].tobytes() == fresh[k][:first].tobytes() and now[k][first + count:].tobytes() == fresh[k][first + count:].tobytes()
    q3.run(35)
    assert_wolf_population_equal(q3.read(first, count), q1.read(first, count))
    # one array alone: the others stay
    q3.load(pi_b=ck["pi_b"], first=first)
    r = q3.read(first, count)
    assert r["pi_b"].tobytes() == ck["pi_b"].tobytes()
    assert_same_bits(r, q1.read(first, count), [k for k in KEYS if k != "pi_b"])
    # a refused load changes nothing (the Python layer checks first, so straight through the ABI)
    before = q3.read()
    nS = b2.nS
    bad_q = ck["Q_a"].copy(); bad_q[count - 1, nS - 1, 4] = 1.5
    bad_pi = ck["pi_a"].copy(); bad_pi[7, 3] = [0.5, 0.5, 0.5, 0.0, 0.0]
    bad_avg = ck["avg_b"].copy(); bad_avg[8, 9, 2] = -0.25
    bad_ds = ck["dscale"].copy(); bad_ds[-1] = 2.0

    def state(**kw):
        return _lib.WolfPopulationState(**{k: x.ctypes.data for k, x in kw.items()})
    for (f, c, st), msg in (((first, count, state(Q_a=bad_q, Q_b=ck["Q_b"])), r"Q_a\[29\]\[%d\]\[4\] is outside" % (nS - 1)),
                            ((first, count, state(Q_a=ck["Q_a"], pi_a=bad_pi)), r"pi_a\[7\]\[3\] does not sum to 1"),
                            ((first, count, state(Q_a=ck["Q_a"], avg_b=bad_avg)), r"avg_b\[8\]\[9\]\[2\] is negative"),
                            ((first, count, state(Q_a=ck["Q_a"], dscale=bad_ds)), r"dscale\[29\]"),
                            ((250, 10, state(Q_a=ck["Q_a"])), "outside the population"),
                            ((-1, 1, state()), "outside the population")):
        assert b2.lib.soccer_wolf_population_load(b2.h, q3.q, f, c, C.byref(st)) == _lib.E_INVALID
        assert re.search(msg, b2.lib.soccer_last_error(b2.h).decode()), (msg, b2.lib.soccer_last_error(b2.h))
        assert_wolf_population_equal(q3.read(), before)
    with pytest.raises(AssertionError, match="\\[-1, 1\\]"):
        q3.load(bad_q, ck["Q_b"], first=first)
    row0 = ck["Q_a"].copy(); row0[:, 0] = 7.0                            # row 0 is taken as zeros
    q3.load(row0, first=first)
    assert (q3.read(first, count)["Q_a"][:, 0] == 0).all()
    b1.close(); b2.close()
    assert q3.q is None and q2.q is None                               # the handle freed both


def test_lanes_that_were_never_reset_contribute_nothing():
    n = 67
    b = SoccerBatch(n, 5, 4, 0.2, seed=SEED, autoreset=True)
    q = b.wolf_population(GAMMA, alpha=0.8, decay=0.5, q_init=0.25, delta_decay=0.25)
    q.run(3)
    r = q.read()
    assert b.misuse() == SoccerBatch.MISUSE_FROZEN and r["steps"] == 3
    assert (r["Q_a"][:, 1:] == 0.25).all() and (r["Q_b"][:, 1:] == 0.25).all() and (r["Q_a"][:, 0] == 0).all()
    assert all((r[k] == 0.2).all() for k in ROWS[2:]) and (r["updates"] == 0).all()
    assert (r["alpha"] == 0.8 * 0.5 * 0.5 * 0.5).all() and (r["dscale"] == 0.25 ** 3).all()
    b.close()


# ---- 6. fixed policies --------------------------------------------------------------------------------------
def test_three_ways_to_a_fixed_policy_agree():
    """after run(40) of a challenger population whose player A is fixed: adopt() from a trained population; a population
    created from read()'s policies through the host path; and a shared fixed policy against the same policy per member"""
    n, T = 67, 40
    kw = dict(RUN_KW)
    b, q = _device_run([30], slip=0.2, n=n, max_steps=100, start=WolfPopulationNumpy(n, 761, GAMMA).load(np.random.default_rng(8)))
    for which in ("pi", "avg"):
        trained = q.read()[which + "_a"]
        assert len({trained[i].tobytes() for i in range(n)}) == n        # the members differ
        ck = b.checkpoint()
        adopted = q.challengers(0, which, **kw)
        ra = adopted.read()
        assert ra["pi_a"].tobytes() == trained.tobytes() and ra["avg_a"].tobytes() == trained.tobytes() and (ra["pi_b"] == 0.2).all()
        adopted.run(T)
        b.restore(ck)
        hosted = b.wolf_population(GAMMA, act_a=trained, act_b="learn", **kw)
        hosted.run(T)
        got, want = adopted.read(), hosted.read()
        assert_wolf_population_equal(got, want)
        assert got["pi_a"].tobytes() == trained.tobytes() and got["avg_a"].tobytes() == trained.tobytes()   # constant under run()
        assert (got["pi_b"] != 0.2).any()
        adopted.close(); hosted.close()
    # one policy for everyone: shared against the same policy given per member
    pol = np.random.default_rng(12).dirichlet(np.ones(5), b.nS)
    ck = b.checkpoint()
    shared = b.wolf_population(GAMMA, act_a="learn", act_b=pol, **kw)
    shared.run(T)
    b.restore(ck)
    each = b.wolf_population(GAMMA, act_a="learn", act_b=np.broadcast_to(pol, (n,) + pol.shape), **kw)
    each.run(T)
    assert_wolf_population_equal(shared.read(), each.read())
    assert (shared.read()["pi_b"] == pol).all()
    with pytest.raises(AssertionError, match="is not SOCCER_PHC_FIXED"):
        shared.adopt(0, q, 0)
    with pytest.raises(AssertionError, match="same population"):
        shared.adopt(1, shared, 1)
    b.close()


def test_a_fixed_player_draws_what_the_host_computed_table_draws():
    """a per-member fixed policy against the restatement, whose rows are the host's thresholds of that policy: the 7x5 run
    case has it; here the shared learner's host-computed table: a one-member population with a fixed A is a soccer_wolf_phc
    learner with that fixed policy on a one-lane handle, bit for bit"""
    T = 60
    for seed in (3, 4):
        b1 = SoccerBatch(1, 5, 4, 0.2, seed=seed, autoreset=True)
        b2 = SoccerBatch(1, 5, 4, 0.2, seed=seed, autoreset=True)
        pol = np.random.default_rng(seed).dirichlet(np.ones(5) * 0.3, b1.nS)     # rows with tiny entries
        q1 = b1.wolf_population(GAMMA, act_a=pol, act_b="learn", **RUN_KW)
        q2 = b2.wolf_phc(GAMMA, act_a=pol, act_b="learn", **RUN_KW)
        b1.reset(); b2.reset()
        q1.run(T); q2.run(T)
        r1, r2 = q1.read(), q2.read()
        for k in ROWS + ("updates",):
            assert r1[k][0].tobytes() == r2[k].tobytes(), k
        assert r1["alpha"][0] == r2["alpha"] and r1["dscale"][0] == r2["dscale"] and r1["steps"] == r2["steps"]
        assert_batches_equal(b1, b2)
        b1.close(); b2.close()


def test_with_both_players_fixed_the_tables_are_a_q_population_s():
    n, T = 67, 40
    b1 = SoccerBatch(n, 5, 4, 0.2, seed=SEED, autoreset=True)
    b2 = SoccerBatch(n, 5, 4, 0.2, seed=SEED, autoreset=True)
    pa = np.random.default_rng(11).dirichlet(np.ones(5), b1.nS); pb = np.random.default_rng(12).dirichlet(np.ones(5), b1.nS)
    q1 = b1.wolf_population(GAMMA, act_a=pa, act_b=pb, **RUN_KW)
    q2 = b2.q_population(GAMMA, act_a=pa, act_b=pb, explor=RUN_KW["explor"], decay=RUN_KW["decay"])
    b1.reset(); b2.reset()
    q1.run(T); q2.run(T)
    r1, r2 = q1.read(), q2.read()
    for k in ("Q_a", "Q_b", "V_a", "V_b", "alpha"):
        assert r1[k].tobytes() == r2[k].tobytes(), k
    assert r1["steps"] == r2["steps"] == T and int(r1["updates"].sum()) == n * T
    assert (r1["pi_a"] == pa).all() and (r1["avg_b"] == pb).all()
    assert_batches_equal(b1, b2)
    b1.close(); b2.close()


# ---- 7. a shared handle, exploitability ---------------------------------------------------------------------
def test_populations_of_both_kinds_and_a_shared_learner_share_a_handle():
    """a WoLF population, a Q-population and a shared-table WoLF-PHC learner alive on one handle, run one after the other from
    the same checkpoint (state and tick): each equals its run alone"""
    T, n = 20, 259
    kw = dict(explor=0.2, decay=0.99)

    def make(b):
        return (b.wolf_population(GAMMA, delta_win=0.1, delta_lose=0.4, **kw), b.q_population(GAMMA, **kw),
                b.wolf_phc(GAMMA, delta_win=0.1, delta_lose=0.4, **kw))
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


def test_exploitability_of_300_members_is_each_member_s_own():
    n = 300
    b = SoccerBatch(n, 5, 4, 0.0, seed=SEED, autoreset=True)
    q = b.wolf_population(GAMMA, **RUN_KW)
    q.load(**WolfPopulationNumpy(n, b.nS, GAMMA).load(np.random.default_rng(9)))
    b.reset(); q.run(100)
    r = q.read()
    for which in ("pi", "avg"):
        e = q.exploitability(which, theta=1e-6)
        assert e["gap"].shape == e["v_a"].shape == e["v_b"].shape == (n, b.nS)
        if which == "pi":
            idx = range(n)
        else:
            idx = (0, 255, 256, 299)                # the chunk boundary
        for i in idx:
            one = pl.exploitability(b, r[which + "_a"][i], r[which + "_b"][i], 1e-6, GAMMA)
            for k in ("v_a", "v_b", "gap"):
                assert e[k][i].tobytes() == one[k].tobytes(), (which, i, k)
        assert (e["gap"][:, 1:] >= -1e-4).all()          # theta / (1 - gamma), with room
    part = q.exploitability("avg", theta=1e-6, first=250, count=7)
    assert part["gap"].tobytes() == e["gap"][250:257].tobytes()
    b.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=False)
    with pytest.raises(AssertionError, match="SOCCER_F_AUTORESET"):
        b.wolf_population(GAMMA)
    b.close()
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=True)
    b.set_policy("player_b", np.zeros(b.nS, np.int8))
    with pytest.raises(AssertionError, match="two-player handle"):
        b.wolf_population(GAMMA)
    b.set_policy("player_b", None)
    q = b.wolf_population(GAMMA)
    with pytest.raises(AssertionError, match="outside the population"):
        q.read(60, 5)
    st = _lib.WolfPopulationState()
    for first, count in ((65, 0), (0, 65), (-1, 2), (3, -1), (2 ** 62, 2 ** 62)):
        assert b.lib.soccer_wolf_population_read(b.h, q.q, first, count, C.byref(st)) == _lib.E_INVALID
        assert "outside the population" in b.lib.soccer_last_error(b.h).decode()
    assert b.lib.soccer_wolf_population_read(b.h, q.q, 0, 1, None) == _lib.E_INVALID and "out is NULL" in b.lib.soccer_last_error(b.h).decode()
    dev = [b.alloc(64, dt).fill(0) for dt in DTYPES]
    fixed_a = b.wolf_population(GAMMA, act_a=np.full((b.nS, 5), 0.2))
    b.sync()
    b.graph_begin()
    b.rollout(2, sample_actions=True)           # (something to capture; never replayed)
    for call in (lambda: q.run(1), lambda: q.read(), lambda: q.load(np.zeros((64, b.nS, 5)), np.zeros((64, b.nS, 5))),
                 lambda: b.wolf_population(GAMMA), lambda: q.update(*dev), lambda: q.steps, lambda: fixed_a.adopt(0, q, 0)):
        with pytest.raises(RuntimeError, match="during graph capture"):
            call()
    b.graph_destroy(b.graph_end())
    other = SoccerBatch(64, 5, 4, 0.0, autoreset=True)
    with pytest.raises(AssertionError, match="not a population of this handle"):
        other._check(other.lib.soccer_wolf_population_run(other.h, q.q, 1))
    foreign = other.wolf_population(GAMMA)
    with pytest.raises(AssertionError, match=r"\(src\): not a population of this handle"):
        fixed_a.adopt(0, foreign, 0)
    other.close()
    for args, msg in (((fixed_a.q, 0, fixed_a.q, 0, 0), "the same population"), ((fixed_a.q, 1, q.q, 0, 0), "player B of dst is not SOCCER_PHC_FIXED"),
                      ((q.q, 0, fixed_a.q, 0, 0), "player A of dst is not SOCCER_PHC_FIXED"), ((fixed_a.q, 2, q.q, 0, 0), "must be 0 .player A. or 1"),
                      ((fixed_a.q, 0, q.q, -1, 0), "must be 0 .player A. or 1"), ((fixed_a.q, 0, q.q, 0, 2), "which must be 0 .pi. or 1 .avg."),
                      ((fixed_a.q, 0, None, 0, 0), "not a population of this handle")):
        assert b.lib.soccer_wolf_population_adopt(b.h, *args) == _lib.E_INVALID
        assert re.search(msg, b.lib.soccer_last_error(b.h).decode()), (msg, b.lib.soccer_last_error(b.h))
    with pytest.raises(AssertionError, match="n_steps must be >= 0"):
        q.run(-1)
    assert b.lib.soccer_wolf_population_update(b.h, q.q, dev[0].ptr, None, None, None, None, None) == _lib.E_INVALID
    # the library's own range checks (the Python layer checks first, so straight through the ABI)
    uniform = np.full((b.nS, 5), 0.2)
    bad_row = uniform.copy(); bad_row[3] = [0.5, 0.5, 0.5, 0.0, 0.0]
    bad_each = np.full((64, b.nS, 5), 0.2); bad_each[41, 17, 2] = float("nan")
    ok64 = np.full(64, 0.5)

    def arr(i, v):
        a = ok64.copy(); a[i] = v
        return a
    keep = [arr(7, 1.0), arr(8, -0.5), arr(9, 0.0), arr(63, 2.0), arr(5, -1.0), arr(6, 1.5), arr(0, 0.0)]
    FIELDS = [f for f, _ in _lib.WolfPopulationConfig._fields_]
    for fields, msg in ((dict(discount_factor=1.0), "discount_factor"), (dict(alpha=-0.5), "alpha"), (dict(decay=0.0), "decay"),
                        (dict(explor=2.0), "explor"), (dict(q_init=-1.5), "q_init"), (dict(delta_win=2.0), "delta_win"),
                        (dict(delta_lose=-1.0), "delta_lose"), (dict(delta_decay=0.0), "delta_decay"), (dict(act_a=7), "act_a"), (dict(act_b=-1), "act_b"),
                        (dict(act_a=_lib.PHC_FIXED), "exactly one of policy_a and policy_a_per_member"),
                        (dict(policy_b=uniform.ctypes.data), "exactly one of policy_b and policy_b_per_member"),
                        (dict(act_a=_lib.PHC_FIXED, policy_a=uniform.ctypes.data, policy_a_per_member=bad_each.ctypes.data), "exactly one of policy_a"),
                        (dict(act_a=_lib.PHC_FIXED, policy_a=bad_row.ctypes.data), "policy_a\\[0\\]\\[3\\] does not sum to 1"),
                        (dict(act_b=_lib.PHC_FIXED, policy_b_per_member=bad_each.ctypes.data), "policy_b_per_member\\[41\\]\\[17\\]\\[2\\] is negative or not a number"),
                        (dict(discount_factor_per_member=keep[0].ctypes.data), "discount_factor_per_member\\[7\\]"),
                        (dict(alpha_per_member=keep[1].ctypes.data), "alpha_per_member\\[8\\]"),
                        (dict(decay_per_member=keep[2].ctypes.data), "decay_per_member\\[9\\]"),
                        (dict(explor_per_member=keep[3].ctypes.data), "explor_per_member\\[63\\]"),
                        (dict(delta_win_per_member=keep[4].ctypes.data), "delta_win_per_member\\[5\\]"),
                        (dict(delta_lose_per_member=keep[5].ctypes.data), "delta_lose_per_member\\[6\\]"),
                        (dict(delta_decay_per_member=keep[6].ctypes.data), "delta_decay_per_member\\[0\\]")):
        cfg = _lib.WolfPopulationConfig(0.9, 1.0, 0.5, 0.2, 1.0, 0.01, 0.04, 1.0, 0, 0)
        for k, v in fields.items():
            assert k in FIELDS
            setattr(cfg, k, v)
        out = C.c_void_p()
        assert b.lib.soccer_wolf_population_create(b.h, C.byref(cfg), C.byref(out)) == _lib.E_INVALID and not out.value
        assert re.search(msg, b.lib.soccer_last_error(b.h).decode()), (msg, b.lib.soccer_last_error(b.h))
    # a per-member array overrides a scalar that is out of range: only what is used is checked
    cfg = _lib.WolfPopulationConfig(0.9, 7.0, 0.5, 0.2, 1.0, 0.01, 0.04, 1.0, 0, 0)
    cfg.alpha_per_member = ok64.ctypes.data
    out = C.c_void_p()
    assert b.lib.soccer_wolf_population_create(b.h, C.byref(cfg), C.byref(out)) == _lib.OK and out.value
    assert b.lib.soccer_wolf_population_destroy(b.h, out) == _lib.OK
    b.reset(); q.run(2); fixed_a.run(2)
    assert q.steps == 2 and fixed_a.steps == 2 and b.tick == 5 and b.misuse() == 0
    b.close()                                   # with live populations: the handle frees them
    assert fixed_a.q is None and q.q is None
    q.close()                                   # the wrapper knows


# ---- 9. it learns -----------------------------------------------------------------------------------------
def test_every_member_learns_the_best_response_values():
    """The learning run of tests/test_wolf_population_np.py on the device, same n, T and seed, so the restatement's figures are
    the device's (test 2 pins the bits): A FIXED uniform, B LEARN, 64 one-actor learners from Q = 0, alpha 1 -> 0.01.  Asserted:
    the population mean of the mean over the live states of |-V_b - V(uniform, B's exact best response)| stays under BOUND (the
    Q side; restatement 0.237436).  Printed beside it: the policy side V(uniform, pi_b) - V(uniform, best response)
    (restatement 0.312553), whose doubled worst case does not lie below the untrained figure at this budget."""
    c = LEARN
    env = VectorSoccerEnv(c["n"], c["width"], c["height"], c["slip"], seed=c["seed"], autoreset=True)
    uniform = np.full((env.nS, 5), 0.2)
    want = pl.best_response(env, uniform, 0, 1e-10, c["gamma"])[1]
    q = env.wolf_population(c["gamma"], alpha=c["alpha"], decay=0.01 ** (1.0 / c["T"]), explor=c["explor"], q_init=c["q_init"],
                            delta_win=c["delta_win"], delta_lose=c["delta_lose"], delta_decay=c["delta_decay"], act_a=uniform, act_b="learn")
    env.reset()
    env._batch.sync()
    t0 = time.perf_counter()
    q.run(c["T"])
    steps = q.steps                             # synchronises
    wall = time.perf_counter() - t0
    r = q.read()
    err = np.abs(-r["V_b"] - want)[:, 1:].mean(1)
    pol = (env._batch.evaluate_policies(uniform, r["pi_b"], 1e-10, c["gamma"])[0] - want)[:, 1:].mean(1)
    print("A uniform, B learns, %d members x %d steps: Q side, population mean %.6f (members %.6f .. %.6f); policy side %.6f (%.6f .. %.6f); "
          "run() took %.3f s = %.2f us per step" % (c["n"], c["T"], err.mean(), err.min(), err.max(), pol.mean(), pol.min(), pol.max(),
                                                    wall, wall / c["T"] * 1e6))
    assert steps == c["T"] and np.abs(r["alpha"] - 0.01).max() < 1e-9
    assert (r["pi_a"] == 0.2).all() and pol.min() >= -1e-9
    assert err.mean() <= BOUND
    out = pl.wolf_population(env, 50, c["gamma"], q_init=0.0, act_a="uniform", first=3, count=5)      # the planner-style entry point
    assert all(x.shape == (5, env.nS, 5) for x in out[:6]) and out[6].shape == (5,)
    assert np.abs(out[1][:, 1:].sum(2) - 1.0).max() < 1e-12
    q.close(); env.close()
