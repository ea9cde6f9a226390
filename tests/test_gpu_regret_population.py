"""-m gpu: the population of regret matchers, a learner per lane (include/soccer_hip.h, "learners, a population of regret
matchers") against its numpy restatement (tests/regret_population_np.py: the oracle as environment), bit for bit — run() from
loaded states on the cases of tests/test_regret_population_np.py (1, 3, 67 and 259 members; 5x4 at slip 0 and 0.2, 7x5 at 0.3;
all four (plus, linear); the four mode pairs; truncating episodes), then the launch split, a capped grid, frozen and parked
lanes, update(), ranges of read and load, the population's size, the refusals and the evaluators.  No tolerances."""
import copy
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
from regret_population_np import ROWS, RegretPopulationNumpy, assert_regret_population_equal  # noqa: E402
from test_learner_edges_np import prepare  # noqa: E402
from test_regret_population_np import GAMMA, RUN_CASES, RUN_IDS, RUN_KW, SEED, T_RUN, act, reference_run  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = (np.uint16, np.int8, np.int8, np.int8, np.uint8, np.uint16)
KEYS = ROWS + ("updates", "alpha")
DERIVED = ("pi_a", "pi_b", "avg_a", "avg_b")


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


def _device_run(parts, w=5, h=4, slip=0.2, act_a="learn", act_b="learn", n=259, max_steps=5, plus=True, linear=False, start=None, **batch_kw):
    """the device twin of reference_run: the same handle, the same loaded state, run(t) for t in parts"""
    if start is None:
        start = reference_run(w, h, slip, act_a, act_b, n, max_steps, plus, linear)[2]
    b = SoccerBatch(n, w, h, slip, seed=SEED, autoreset=True, max_steps=max_steps, **batch_kw)
    q = b.regret_population(GAMMA, plus=plus, linear=linear, act_a=act(act_a, n, b.nS), act_b=act(act_b, n, b.nS), **RUN_KW)
    q.load(**start)
    b.reset()
    for t in parts:
        q.run(t)
    return b, q


# ---- 1. run(60) from a loaded state against the restatement, exactly -------------------------------------------------------
@pytest.mark.parametrize("case", RUN_CASES, ids=RUN_IDS)
def test_run_equals_the_restatement_bit_for_bit(case):
    w, h, slip, act_a, act_b, n, max_steps, plus, linear = case
    o, ref, start = reference_run(*case)
    b, q = _device_run([T_RUN], *case)
    got = q.read()
    assert_regret_population_equal(got, ref.state())
    assert_same_bits(got, ref.derived(), DERIVED)                    # read()'s expressions are the device's
    assert_state_equal(b, o)
    assert b.tick == o.tick == T_RUN + 1
    hist, misuse = b.stats()
    np.testing.assert_array_equal(hist, o.hist)
    assert misuse == 0 and ref.n_left_out == 0 and ref.n_uniform > 0 and (ref.n_floor > 0) == plus
    assert q.steps == T_RUN and (q.alpha == ref.alpha).all() and (q.plus, q.linear) == (plus, linear)
    part = q.read(n // 2, 1)                                          # a range is the slice
    assert_same_bits(part, ref.state(n // 2, 1)); assert_same_bits(part, ref.derived(n // 2, 1), DERIVED)
    b.close()


def test_a_fresh_population_is_what_creation_defines():
    b = SoccerBatch(67, 5, 4, 0.0, seed=SEED, autoreset=True)
    q = b.regret_population(GAMMA, q_init=0.25, alpha=0.5)
    r = q.read()
    assert (r["Q_a"][:, 1:] == 0.25).all() and (r["Q_b"][:, 1:] == 0.25).all() and (r["Q_a"][:, 0] == 0).all() and (r["Q_b"][:, 0] == 0).all()
    assert all(not r[k].view(np.uint64).any() for k in ROWS[2:]) and not r["updates"].any() and (r["alpha"] == 0.5).all() and r["steps"] == 0
    assert all((r[k] == 0.2).all() for k in DERIVED)
    assert_regret_population_equal(r, RegretPopulationNumpy(67, b.nS, GAMMA, q_init=0.25, alpha=0.5).state())
    b.close()


# ---- 2. the launch split, the capped grid -------------------------------------------------------------------------------------
def test_result_does_not_depend_on_the_steps_per_launch(monkeypatch):
    """slip 0: a Philox block spans eight ticks, so with seven steps per launch a launch starts in the middle of a block"""
    args = dict(slip=0.0, act_b="uniform", n=67, max_steps=5, plus=True, linear=True)
    start = reference_run(5, 4, 0.0, "learn", "uniform", 67, 5, True, True, T=20)[2]
    b1, q1 = _device_run([20], start=start, **args)                   # one launch
    b3, q3 = _device_run([7, 7, 6], start=start, **args)
    monkeypatch.setenv("SOCCER_POP_LAUNCH_STEPS", "7")
    b2, q2 = _device_run([20], start=start, **args)                   # 7 + 7 + 6 inside one call
    monkeypatch.delenv("SOCCER_POP_LAUNCH_STEPS")
    want = reference_run(5, 4, 0.0, "learn", "uniform", 67, 5, True, True, T=20)[1]
    for b, q in ((b1, q1), (b2, q2), (b3, q3)):
        assert_regret_population_equal(q.read(), want.state())
        assert_batches_equal(b, b1)
        assert q.steps == 20 and b.tick == 21
    b1.close(); b2.close(); b3.close()


def test_a_thread_that_serves_several_members(monkeypatch):
    """two workgroups of 256 threads for 777 members: a thread takes up to two members in turn, the last round is ragged"""
    case = (5, 4, 0.2, "learn", "each", 777, 5, True, True)
    o, ref, start = reference_run(*case, T=20)
    ref = copy.deepcopy(ref)                                            # (update() below moves it: the shared reference stays)
    monkeypatch.setenv("SOCCER_POP_GRID_BLOCKS", "2")
    b, q = _device_run([20], *case, start=start)
    monkeypatch.delenv("SOCCER_POP_GRID_BLOCKS")
    assert_regret_population_equal(q.read(), ref.state())
    assert_state_equal(b, o)
    np.testing.assert_array_equal(b.stats()[0], o.hist)
    upd = [b.alloc(777, dt).upload(np.ascontiguousarray(x, dt)) for x, dt in zip(_valid(np.random.default_rng(5), b.nS, 777), DTYPES)]
    q.update(*upd); ref.update(*_valid(np.random.default_rng(5), b.nS, 777))      # update()'s loop wraps too
    assert_regret_population_equal(q.read(), ref.state())
    b.close()


# ---- 3. frozen and parked lanes -----------------------------------------------------------------------------------------------
def test_frozen_and_parked_lanes_leave_their_rows_alone_and_still_advance_alpha():
    n, T = 67, 12
    c = dict(n=n, special="mix", max_steps=100)
    o = Oracle(5, 4, 0.2, n=n, seed=SEED, autoreset=True, max_steps=100)
    obs, st, m = prepare(c, o)
    ref = RegretPopulationNumpy(n, o.nS, GAMMA, plus=True, linear=True, **RUN_KW)
    start = ref.load(np.random.default_rng(21))
    ref.run(o, obs, T)
    assert m["frozen"].sum() > 0 and m["parked"].sum() > 0 and ref.n_left_out == int(m["frozen"].sum()) * T + int(m["parked"].sum())
    b = SoccerBatch(n, 5, 4, 0.2, seed=SEED, autoreset=True, max_steps=100)
    q = b.regret_population(GAMMA, plus=True, linear=True, **RUN_KW)
    q.load(**start)
    b.reset(); b.set_state(**st)
    q.run(1)
    first = q.read()
    for i in np.flatnonzero(m["parked"] | m["frozen"]):              # the parked lanes' first step, at observation 0, moved nothing
        assert_same_bits({k: first[k][i] for k in ROWS + ("updates",)}, {k: start[k][i] for k in ROWS + ("updates",)}, ROWS + ("updates",), i)
    q.run(T - 1)
    got = q.read()
    assert_regret_population_equal(got, ref.state())
    assert_state_equal(b, o)
    assert b.misuse() == SoccerBatch.MISUSE_FROZEN and got["steps"] == T
    for i in np.flatnonzero(m["frozen"]):                            # rows untouched, alpha advanced T times
        assert_same_bits({k: got[k][i] for k in ROWS + ("updates",)}, {k: start[k][i] for k in ROWS + ("updates",)}, ROWS + ("updates",), i)
    assert (got["alpha"] == ref.alpha).all() and len(set(got["alpha"].tolist())) == 1 and got["alpha"][0] < RUN_KW["alpha"]
    assert not got["updates"][:, 0].any() and all(not got[k][:, 0].view(np.uint64).any() for k in ROWS)      # row 0 never moves
    b.close()


# ---- 4. update() ------------------------------------------------------------------------------------------------------------
def _valid(rng, nS, n):
    """obs, act_a, act_b, reward, terminated, next_obs; a reward is non-zero only on a terminated transition"""
    obs = rng.integers(1, nS, n); term = rng.random(n) < 0.3
    nxt = np.where(term, 0, rng.integers(0, nS, n))
    rew = np.where(term, rng.choice([-1, 1], n), 0)
    return [obs, rng.integers(0, 5, n), rng.integers(0, 5, n), rew, term.astype(np.uint8), nxt]


@pytest.mark.parametrize("plus, linear, act_b", [(True, False, "learn"), (False, True, "each")], ids=["plus learn-learn", "linear learn-fixed"])
def test_update_equals_numpy_bit_for_bit_and_leaves_bad_transitions_out(plus, linear, act_b):
    n = 67
    b = SoccerBatch(n, 5, 4, 0.0, seed=1, autoreset=True)
    nS = b.nS
    kw = dict(alpha=0.75, decay=0.9, explor=0.2, q_init=0.5, plus=plus, linear=linear, act_b=act(act_b, n, nS))
    q = b.regret_population(GAMMA, **kw)
    ref = RegretPopulationNumpy(n, nS, GAMMA, **kw)
    assert_regret_population_equal(q.read(), ref.state())
    q.load(**ref.load(np.random.default_rng(2)))
    assert_regret_population_equal(q.read(), ref.state())
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
    tick = b.tick
    for batch, kp, flags in ((warm, None, 0), (case, keep, SoccerBatch.MISUSE_ACTION | SoccerBatch.MISUSE_OBSERVATION), (warm, None, 0)):
        before = q.read()
        q.update(*batch)
        ref.update(*batch, keep=kp)
        got = q.read()
        assert_regret_population_equal(got, ref.state())
        assert b.misuse() == flags
        b.reset_stats()
        if kp is not None:
            for i in bad_act + bad_obs:             # flag raised, that member's rows unchanged, alpha advanced
                assert_same_bits({k: got[k][i] for k in ROWS + ("updates",)}, {k: before[k][i] for k in ROWS + ("updates",)}, ROWS + ("updates",), i)
                assert got["alpha"][i] == before["alpha"][i] * 0.9
        assert ((got["updates"] != before["updates"]).sum(1) <= 1).all() and (got["Q_a"][:, 0] == 0).all() and (got["Q_b"][:, 0] == 0).all()
    assert q.steps == 3 and (q.alpha == ref.alpha).all() and b.tick == tick
    assert ref.n_uniform > 0 and (ref.n_floor > 0) == plus
    dev = [b.alloc(n, dt).upload(np.ascontiguousarray(x, dt)) for x, dt in zip(warm, DTYPES)]       # device arrays in
    q.update(*dev); ref.update(*warm)
    assert_regret_population_equal(q.read(), ref.state())
    with pytest.raises(AssertionError, match="one transition per member"):
        q.update(*[x[:5] for x in warm])
    q.close(); b.close()


# ---- 5. read and load of ranges ---------------------------------------------------------------------------------------------
def test_read_then_load_of_a_range_on_a_fresh_population_continues_the_same():
    first, count = 10, 30
    case = dict(plus=False, linear=True)
    b1, q1 = _device_run([40], **case)
    b2, q2 = _device_run([15], **case)
    ck = q2.read(first, count)
    q3 = b2.regret_population(GAMMA, **case, **RUN_KW)                 # a second, fresh population on the same handle
    fresh = q3.read()
    q3.load(**{k: ck[k] for k in KEYS + ("steps",)}, first=first)
    now = q3.read()
    assert_regret_population_equal(q3.read(first, count), ck)
    for k in KEYS:                                                     # nothing outside the range moved
        assert now[k][:first].tobytes() == fresh[k][:first].tobytes() and now[k][first + count:].tobytes() == fresh[k][first + count:].tobytes()
    q3.run(25)
    assert_regret_population_equal(q3.read(first, count), q1.read(first, count))
    # one array alone: the others stay
    q3.load(Z_b=ck["Z_b"], first=first)
    r = q3.read(first, count)
    assert r["Z_b"].tobytes() == ck["Z_b"].tobytes()
    assert_same_bits(r, q1.read(first, count), [k for k in KEYS if k != "Z_b"])
    # a refused load changes nothing (the Python layer checks first, so straight through the ABI)
    before = q3.read()
    nS = b2.nS
    bad_q = ck["Q_a"].copy(); bad_q[count - 1, nS - 1, 4] = 1.5
    bad_r = ck["R_a"].copy(); bad_r[7, 3, 1] = float("nan")
    bad_z = ck["Z_b"].copy(); bad_z[8, 9, 2] = -0.25
    bad_al = ck["alpha"].copy(); bad_al[-1] = 2.0

    def state(**kw):
        return _lib.RegretPopulationState(**{k: x.ctypes.data for k, x in kw.items()})
    for (f, c, st), msg in (((first, count, state(Q_a=bad_q, Q_b=ck["Q_b"])), r"Q_a\[29\]\[%d\]\[4\] is outside" % (nS - 1)),
                            ((first, count, state(Q_a=ck["Q_a"], R_a=bad_r)), r"R_a\[7\]\[3\]\[1\] is not a finite number"),
                            ((first, count, state(Q_a=ck["Q_a"], Z_b=bad_z)), r"Z_b\[8\]\[9\]\[2\] is negative or not a finite number"),
                            ((first, count, state(Q_a=ck["Q_a"], alpha=bad_al)), r"alpha\[29\]"),
                            ((250, 10, state(Q_a=ck["Q_a"])), "outside the population"),
                            ((-1, 1, state()), "outside the population")):
        assert b2.lib.soccer_regret_population_load(b2.h, q3.q, f, c, C.byref(st)) == _lib.E_INVALID
        assert re.search(msg, b2.lib.soccer_last_error(b2.h).decode()), (msg, b2.lib.soccer_last_error(b2.h))
        assert_regret_population_equal(q3.read(), before)
    assert b2.lib.soccer_regret_population_load(b2.h, q3.q, 0, 1, None) == _lib.E_INVALID and "in is NULL" in b2.lib.soccer_last_error(b2.h).decode()
    with pytest.raises(AssertionError, match="\\[-1, 1\\]"):
        q3.load(bad_q, ck["Q_b"], first=first)
    with pytest.raises(AssertionError, match="Z_b must be finite and >= 0"):
        q3.load(Z_b=bad_z, first=first)
    row0 = ck["Q_a"].copy(); row0[:, 0] = 7.0                            # row 0 is taken as zeros
    q3.load(row0, first=first)
    assert (q3.read(first, count)["Q_a"][:, 0] == 0).all()
    # under plus a negative regret is refused by the library too
    q4 = b2.regret_population(GAMMA, plus=True)
    neg = np.zeros((1, nS, 5)); neg[0, 5, 0] = -1e-3
    assert b2.lib.soccer_regret_population_load(b2.h, q4.q, 3, 1, C.byref(state(R_b=neg))) == _lib.E_INVALID
    assert re.search(r"R_b\[0\]\[5\]\[0\] is negative or not a finite number", b2.lib.soccer_last_error(b2.h).decode())
    b1.close(); b2.close()
    assert q3.q is None and q2.q is None and q4.q is None              # the handle freed them


# ---- 6. the population's size -------------------------------------------------------------------------------------------------
def test_member_i_of_259_is_the_one_member_population_on_lane_i():
    """a lane's stream depends on its global index alone, and a member on its lane alone: a handle of one lane at lane_offset i,
    loaded with member i's rows, is member i of the 259"""
    case = (5, 4, 0.2, "learn", "learn", 259, 5, True, True)
    start = reference_run(*case)[2]
    b, q = _device_run([T_RUN], *case)
    got = q.read()
    for i in (0, 63, 64, 255, 256, 258):
        b1, q1 = _device_run([T_RUN], 5, 4, 0.2, "learn", "learn", 1, 5, True, True, start={k: v[i:i + 1] for k, v in start.items()}, lane_offset=i)
        one = q1.read()
        assert_same_bits({k: one[k][0] for k in KEYS}, {k: got[k][i] for k in KEYS}, where=i)
        assert one["steps"] == got["steps"]
        b1.close()
    b.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_consume_no_tick():
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=False)
    with pytest.raises(AssertionError, match="SOCCER_F_AUTORESET"):
        b.regret_population(GAMMA)
    b.close()
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=True)
    b.set_policy("player_b", np.zeros(b.nS, np.int8))
    with pytest.raises(AssertionError, match="two-player handle"):
        b.regret_population(GAMMA)
    b.set_policy("player_b", None)
    q = b.regret_population(GAMMA)
    with pytest.raises(AssertionError, match="outside the population"):
        q.read(60, 5)
    st = _lib.RegretPopulationState()
    for first, count in ((65, 0), (0, 65), (-1, 2), (3, -1), (2 ** 62, 2 ** 62)):
        assert b.lib.soccer_regret_population_read(b.h, q.q, first, count, C.byref(st)) == _lib.E_INVALID
        assert "outside the population" in b.lib.soccer_last_error(b.h).decode()
    assert b.lib.soccer_regret_population_read(b.h, q.q, 0, 1, None) == _lib.E_INVALID and "out is NULL" in b.lib.soccer_last_error(b.h).decode()
    dev = [b.alloc(64, dt).fill(0) for dt in DTYPES]
    b.sync()
    b.graph_begin()
    b.rollout(2, sample_actions=True)           # (something to capture; never replayed)
    for call in (lambda: q.run(1), lambda: q.read(), lambda: q.load(np.zeros((64, b.nS, 5)), np.zeros((64, b.nS, 5))),
                 lambda: b.regret_population(GAMMA), lambda: q.update(*dev), lambda: q.steps):
        with pytest.raises(RuntimeError, match="during graph capture"):
            call()
    b.graph_destroy(b.graph_end())
    b.reset()
    tick = b.tick
    other = SoccerBatch(64, 5, 4, 0.0, autoreset=True)
    with pytest.raises(AssertionError, match="not a population of this handle"):
        other._check(other.lib.soccer_regret_population_run(other.h, q.q, 1))
    wolf = b.wolf_population(GAMMA)             # another kind's handle is no regret population
    with pytest.raises(AssertionError, match="not a population of this handle"):
        b._check(b.lib.soccer_regret_population_run(b.h, wolf.q, 1))
    other.close()
    with pytest.raises(AssertionError, match="n_steps must be >= 0"):
        q.run(-1)
    assert b.lib.soccer_regret_population_update(b.h, q.q, dev[0].ptr, None, None, None, None, None) == _lib.E_INVALID
    assert "all six transition arrays" in b.lib.soccer_last_error(b.h).decode()
    # the library's own checks of a config (the Python layer checks first, so straight through the ABI)
    uniform = np.full((b.nS, 5), 0.2)
    bad_row = uniform.copy(); bad_row[3] = [0.5, 0.5, 0.5, 0.0, 0.0]
    bad_each = np.full((64, b.nS, 5), 0.2); bad_each[41, 17, 2] = float("nan")
    ok64 = np.full(64, 0.5)

    def arr(i, v):
        a = ok64.copy(); a[i] = v
        return a
    keep = [arr(7, 1.0), arr(8, -0.5), arr(9, 0.0), arr(63, 2.0)]
    FIELDS = [f for f, _ in _lib.RegretPopulationConfig._fields_]
    for fields, msg in ((dict(discount_factor=1.0), "discount_factor"), (dict(alpha=-0.5), "alpha"), (dict(decay=0.0), "decay"),
                        (dict(explor=2.0), "explor"), (dict(q_init=-1.5), "q_init"), (dict(act_a=7), "act_a"), (dict(act_b=-1), "act_b"),
                        (dict(plus=2), "plus / linear must be 0 or 1"), (dict(linear=-1), "plus / linear must be 0 or 1"),
                        (dict(act_a=_lib.PHC_FIXED), "exactly one of policy_a and policy_a_per_member"),
                        (dict(policy_b=uniform.ctypes.data), "exactly one of policy_b and policy_b_per_member"),
                        (dict(act_a=_lib.PHC_FIXED, policy_a=uniform.ctypes.data, policy_a_per_member=bad_each.ctypes.data), "exactly one of policy_a"),
                        (dict(act_a=_lib.PHC_FIXED, policy_a=bad_row.ctypes.data), "policy_a\\[0\\]\\[3\\] does not sum to 1"),
                        (dict(act_b=_lib.PHC_FIXED, policy_b_per_member=bad_each.ctypes.data), "policy_b_per_member\\[41\\]\\[17\\]\\[2\\] is negative or not a number"),
                        (dict(discount_factor_per_member=keep[0].ctypes.data), "discount_factor_per_member\\[7\\]"),
                        (dict(alpha_per_member=keep[1].ctypes.data), "alpha_per_member\\[8\\]"),
                        (dict(decay_per_member=keep[2].ctypes.data), "decay_per_member\\[9\\]"),
                        (dict(explor_per_member=keep[3].ctypes.data), "explor_per_member\\[63\\]")):
        cfg = _lib.RegretPopulationConfig(0.9, 1.0, 0.5, 0.2, 1.0, 0, 0, 1, 0)
        for k, v in fields.items():
            assert k in FIELDS
            setattr(cfg, k, v)
        out = C.c_void_p()
        assert b.lib.soccer_regret_population_create(b.h, C.byref(cfg), C.byref(out)) == _lib.E_INVALID and not out.value
        assert re.search(msg, b.lib.soccer_last_error(b.h).decode()), (msg, b.lib.soccer_last_error(b.h))
    assert b.tick == tick and q.steps == 0 and b.misuse() == 0          # nothing above consumed a tick or ran a step
    q.run(2); wolf.run(1)
    assert q.steps == 2 and b.tick == tick + 3 and b.misuse() == 0
    b.close()                                   # with live populations: the handle frees them
    assert q.q is None and wolf.q is None
    q.close()                                   # the wrapper knows


# ---- 8. the evaluators ----------------------------------------------------------------------------------------------------------
def _same(a, b, where):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), where
        for k in a:
            _same(a[k], b[k], (where, k))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, (where, i))
    elif isinstance(a, np.ndarray):
        assert a.tobytes() == np.asarray(b).tobytes(), where
    else:
        assert a == b, where


def test_the_evaluators_are_the_batch_s_calls_on_what_read_returns():
    case = (5, 4, 0.2, "learn", "learn", 67, 100, True, True)
    b, q = _device_run([T_RUN], *case)
    first, count, theta = 30, 5, 1e-6
    r = q.read(first, count)
    assert (r["avg_a"] != r["pi_a"]).any() and np.abs(r["avg_b"].sum(2) - 1.0).max() < 1e-12
    for which in ("avg", "pi"):
        pa, pb = r[which + "_a"], r[which + "_b"]
        e = q.exploitability(which, theta=theta, first=first, count=count)
        one = pl.exploitability(b, pa, pb, theta, GAMMA)
        for k in ("v_a", "v_b", "gap"):
            assert e[k].tobytes() == one[k].tobytes(), (which, k)
        _same(q.cross_play(which, theta, first, count), b.cross_play(pa, pb, theta, GAMMA), (which, "cross_play"))
        _same(q.match_outcomes(which, theta, first, count), b.match_outcomes(pa, pb, theta, GAMMA), (which, "match_outcomes"))
        _same(q.occupancy(which, theta, first, count), b.occupancy(pa, pb, theta, GAMMA), (which, "occupancy"))
        m = q.meta_game(which, theta, first, count)
        want = pl.meta_game(b, pa, pb, theta, GAMMA)
        for k in ("payoff", "x", "y", "value", "lo", "hi", "status"):
            _same(m[k], want[k], (which, "meta_game", k))
    # 'avg' is the default pair
    assert q.exploitability(theta=theta, first=first, count=count)["gap"].tobytes() == q.exploitability("avg", theta, first, count)["gap"].tobytes()
    assert q.cross_play(theta=theta, first=first, count=count)[0].tobytes() == q.cross_play("avg", theta, first, count)[0].tobytes()
    with pytest.raises(AssertionError, match="which must be 'avg' or 'pi'"):
        q.cross_play("greedy")
    b.close()


def test_the_planner_style_entry_point_and_the_env_s_factory():
    env = VectorSoccerEnv(64, 5, 4, 0.0, seed=SEED, autoreset=True)
    out = pl.regret_population(env, 50, GAMMA, q_init=0.0, act_b="uniform", first=3, count=5)
    assert all(x.shape == (5, env.nS, 5) for x in out[:6]) and out[6].shape == (5,)
    assert np.abs(out[0].sum(2) - 1.0).max() < 1e-12 and (out[1] == 0.2).all() and (out[3] == 0.2).all()
    q = env.regret_population(GAMMA, linear=True)
    assert q.linear and q.plus and q.read(0, 1)["Q_a"].shape == (1, env.nS, 5)
    q.close(); env.close()
