"""-m gpu: the independent Q-learners on the device (include/soccer_hip.h, "learners, independent Q") against their numpy
restatement (tests/q_learning_np.py: the oracle as environment), bit for bit — update() on synthetic batches, run() on four
pitches; then composition and invariance, the refusals, and the learning test against the exact best response."""
import os
import re
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch, VectorSoccerEnv
from gym_soccer_littman94_amd import planners as pl
from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from q_learning_np import QLearningNumpy, assert_learner_equal, behaviour  # noqa: E402
from test_q_learning_np import BOUND  # noqa: E402

pytestmark = pytest.mark.gpu

GAMMA = 0.9
DTYPES = (np.uint16, np.int8, np.int8, np.int8, np.uint8, np.uint16)


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


# ---- 1. update() against numpy, exactly ---------------------------------------------------------------
def _random_batch(rng, nS, n):
    obs = rng.integers(1, nS, n); term = rng.random(n) < 0.3
    nxt = np.where(term, 0, rng.integers(0, nS, n))
    rew = np.where(term, rng.choice([-1, 1], n), 0)
    return obs, rng.integers(0, 5, n), rng.integers(0, 5, n), rew, term.astype(np.uint8), nxt


def _batches(nS):
    """obs, act_a, act_b, reward, terminated, next_obs; a reward is non-zero only on a terminated transition"""
    rng = np.random.default_rng(1994)

    def one(n, s, a, b, rew):
        rew = np.asarray(rew)
        return np.full(n, s), np.full(n, a), np.broadcast_to(b, (n,)).copy(), rew, (rew != 0).astype(np.uint8), np.where(rew != 0, 0, rng.integers(1, nS, n))
    n = 65536
    return {
        "random cells": _random_batch(rng, nS, 5000),
        "one row, 65536 samples over all b": one(n, 17, 3, rng.integers(0, 5, n), np.where(rng.random(n) < 0.1, rng.choice([-1, 1], n), 0)),
        "terminated, next_obs 0": one(300, 5, 0, 4, np.ones(300, np.int64)),
        "rewards of both signs in one cell": one(1001, nS - 1, 4, 4, rng.choice([-1, 0, 1], 1001)),
        "n = 1": one(1, 9, 2, 2, np.array([-1])),
    }


@pytest.mark.parametrize("case", ["random cells", "one row, 65536 samples over all b", "terminated, next_obs 0",
                                  "rewards of both signs in one cell", "n = 1"])
def test_update_equals_numpy_bit_for_bit(case):
    b = SoccerBatch(8, 5, 4, 0.0, seed=1, autoreset=True)
    kw = dict(alpha=0.75, decay=0.9, explor=0.2, q_init=0.5)
    q = b.q_learning(GAMMA, **kw)
    ref = QLearningNumpy(b.nS, GAMMA, **kw)
    assert_learner_equal(q.read(), ref.state())
    warm = _random_batch(np.random.default_rng(7), b.nS, 20000)      # the values leave their initial constant
    for batch in (warm, _batches(b.nS)[case], warm):
        before = q.read()
        q.update(*batch)
        ref.update(*batch)
        got = q.read()
        assert_learner_equal(got, ref.state())
        untouched = np.setdiff1d(np.arange(b.nS), np.unique(batch[0]))
        for k in ("Q_a", "Q_b", "visits"):
            assert got[k][untouched].tobytes() == before[k][untouched].tobytes(), k
    assert q.steps == 3 and q.alpha == ref.alpha
    assert b.misuse() == 0
    dev = [b.alloc(len(x), dt).upload(x) for x, dt in zip(warm, DTYPES)]       # device arrays in
    q.update(*dev); ref.update(*warm)
    assert_learner_equal(q.read(), ref.state())
    q.update(*[np.zeros(0)] * 6); ref.update(*[np.zeros(0, np.int64)] * 6)      # n = 0: alpha and the counter alone
    assert_learner_equal(q.read(), ref.state())
    q.close(); b.close()


def test_update_leaves_bad_transitions_out_and_flags_them():
    b = SoccerBatch(8, 5, 4, 0.0, seed=1, autoreset=True)
    q = b.q_learning(GAMMA, q_init=0.25)
    ref = QLearningNumpy(b.nS, GAMMA, q_init=0.25)
    good = _random_batch(np.random.default_rng(3), b.nS, 4000)
    bad_act = [x.copy() for x in good]; bad_act[1][::7] = 5; bad_act[2][3::11] = -1
    keep = np.ones(4000, bool); keep[::7] = False; keep[3::11] = False
    q.update(*bad_act); ref.update(*[x[keep] for x in good])
    assert_learner_equal(q.read(), ref.state())
    assert b.misuse() == SoccerBatch.MISUSE_ACTION
    b.reset_stats()
    bad_obs = [x.copy() for x in good]; bad_obs[0][::5] = 0; bad_obs[0][1::9] = b.nS; bad_obs[5][2::13] = b.nS + 3
    keep = np.ones(4000, bool); keep[::5] = False; keep[1::9] = False; keep[2::13] = False
    q.update(*bad_obs); ref.update(*[x[keep] for x in good])
    assert_learner_equal(q.read(), ref.state())
    assert b.misuse() == SoccerBatch.MISUSE_OBSERVATION
    b.reset_stats()
    before = q.read()                   # nothing but bad transitions: alpha and the step counter move, nothing else does
    q.update(*[np.zeros(10)] * 6)
    after = q.read()
    for k in ("Q_a", "Q_b", "visits"):
        assert after[k].tobytes() == before[k].tobytes()
    assert after["steps"] == before["steps"] + 1 and b.misuse() == SoccerBatch.MISUSE_OBSERVATION
    b.close()


# ---- 2. run(T) against the restatement, exactly --------------------------------------------------------
N_RUN, T_RUN, SEED = 8192 + 3, 60, 1994
RUN_KW = dict(explor=0.2, decay=0.99)


def _act(name, nS):
    if name == "dirichlet":
        return np.random.default_rng(11).dirichlet(np.ones(5), nS)
    return name


_REFERENCE = {}


def _reference_run(w, h, slip, act_a, act_b, T=T_RUN, n=N_RUN):
    """computed once per case and left unchanged"""
    key = (w, h, slip, act_a, act_b, T, n)
    if key not in _REFERENCE:
        o = Oracle(w, h, slip, n=n, seed=SEED, autoreset=True)
        ref = QLearningNumpy(o.nS, GAMMA, act_a=_act(act_a, o.nS), act_b=_act(act_b, o.nS), **RUN_KW)
        ref.run(o, o.reset(), T)
        _REFERENCE[key] = (o, ref)
    return _REFERENCE[key]


@pytest.mark.parametrize("w,h,slip,act_a,act_b", [(5, 4, 0.0, "greedy", "uniform"), (5, 4, 0.2, "greedy", "greedy"),
                                                  (7, 5, 0.3, "dirichlet", "greedy"), (11, 7, 0.2, "uniform", "greedy")])
def test_run_equals_the_restatement_bit_for_bit(w, h, slip, act_a, act_b):
    o, ref = _reference_run(w, h, slip, act_a, act_b)
    b = SoccerBatch(N_RUN, w, h, slip, seed=SEED, autoreset=True)
    q = b.q_learning(GAMMA, act_a=_act(act_a, b.nS), act_b=_act(act_b, b.nS), **RUN_KW)
    b.reset()
    q.run(T_RUN)
    assert_learner_equal(q.read(), ref.state())
    assert_state_equal(b, o)
    assert b.tick == o.tick == T_RUN + 1
    hist, misuse = b.stats()
    np.testing.assert_array_equal(hist, o.hist)
    assert misuse == 0 and hist.sum() > 0
    assert q.steps == T_RUN and q.alpha == ref.alpha
    b.close()


# ---- 3. composition and invariance ----------------------------------------------------------------------
def _device_run(parts, w=5, h=4, slip=0.2, act_a="greedy", act_b="greedy", n=N_RUN):
    b = SoccerBatch(n, w, h, slip, seed=SEED, autoreset=True)
    q = b.q_learning(GAMMA, act_a=act_a, act_b=act_b, **RUN_KW)
    b.reset()
    for t in parts:
        q.run(t)
    return b, q


def test_runs_compose_and_repeat():
    b1, q1 = _device_run([60]); b2, q2 = _device_run([25, 35]); b3, q3 = _device_run([60])
    r1 = q1.read()
    assert_learner_equal(q2.read(), r1); assert_learner_equal(q3.read(), r1)
    assert_batches_equal(b1, b2); assert_batches_equal(b1, b3)
    assert_learner_equal(r1, _reference_run(5, 4, 0.2, "greedy", "greedy")[1].state())
    for b in (b1, b2, b3):
        b.close()


@pytest.mark.parametrize("var,value", [("SOCCER_SWAR_LAUNCH_LANES", "4096"), ("SOCCER_STATE_LAYOUT", "wide")])
def test_result_does_not_depend_on_launch_split_or_state_layout(var, value, monkeypatch):
    b1, q1 = _device_run([40])
    monkeypatch.setenv(var, value)
    b2, q2 = _device_run([40])
    monkeypatch.delenv(var)
    if var == "SOCCER_STATE_LAYOUT":
        assert b1.state_streams() == 3 and b2.state_streams() == 6
    assert_learner_equal(q2.read(), q1.read())
    assert_batches_equal(b1, b2)
    b1.close(); b2.close()


def test_run_is_rollout_plus_update_step_by_step():
    """run(T) = T x [the 1-step mixed-policy rollout with both players' epsilon-greedy rows, recording obs / final_obs / reward /
    terminated, the actions recomputed with the oracle's draw, then update()]"""
    T, n = 12, 4096 + 3
    b1, q1 = _device_run([T], slip=0.0, n=n)
    b2 = SoccerBatch(n, 5, 4, 0.0, seed=SEED, autoreset=True)
    q2 = b2.q_learning(GAMMA, **RUN_KW)
    o = Oracle(5, 4, 0.0, n=n, seed=SEED, autoreset=True)              # its action draw only
    obs_d = b2.alloc(n, np.uint16); fin_d = b2.alloc(n, np.uint16); rew_d = b2.alloc(n, np.int8); term_d = b2.alloc(n, np.uint8)
    mix_a = b2.alloc((b2.nS, 4), np.uint16); mix_b = b2.alloc((b2.nS, 4), np.uint16)
    b2.reset(obs=obs_d)
    obs = obs_d.download()
    for _ in range(T):
        r = q2.read()
        ma, mb = behaviour(r["pi_a"], 0.2), behaviour(r["pi_b"], 0.2)
        mix_a.upload(ma); mix_b.upload(mb)
        o.tick = b2.tick
        a, bb = o.sample_actions_mixed(obs, ma, mb)
        b2.rollout(1, sample_actions=True, mix_a=mix_a, mix_b=mix_b, obs=obs_d, reward=rew_d, terminated=term_d, final_obs=fin_d,
                   out_stride=(n + 3) & ~3)
        q2.update(obs, a, bb, rew_d.download(), term_d.download(), fin_d.download())
        obs = obs_d.download()
    assert_learner_equal(q2.read(), q1.read())
    assert_batches_equal(b1, b2)
    b1.close(); b2.close()


def test_read_then_load_on_a_fresh_learner_continues_the_same():
    b1, q1 = _device_run([60])
    b2, q2 = _device_run([25])
    ck = q2.read()
    q3 = b2.q_learning(GAMMA, **RUN_KW)                                # a second learner on the same handle
    q3.load(ck["Q_a"], ck["Q_b"], visits=ck["visits"], alpha=ck["alpha"], steps=ck["steps"])
    assert_learner_equal(q3.read(), ck)
    q3.run(35)
    assert_learner_equal(q3.read(), q1.read())
    q4 = b2.q_learning(GAMMA, **RUN_KW)                                # without the counts they are zeroed
    q4.load(ck["Q_a"], ck["Q_b"])
    r4 = q4.read()
    assert r4["Q_a"].tobytes() == ck["Q_a"].tobytes() and r4["Q_b"].tobytes() == ck["Q_b"].tobytes() and (r4["visits"] == 0).all()
    with pytest.raises(AssertionError, match="\\[-1, 1\\]"):
        q4.load(ck["Q_a"] + 2.0, ck["Q_b"])
    b1.close(); b2.close()


def test_a_minimax_q_learner_and_a_q_learner_share_a_handle():
    """both alive on one handle, run one after the other from the same checkpoint (state and tick), and their update()s
    interleaved: each equals its run alone"""
    T, n = 20, 4096 + 3
    kw = dict(explor=0.2, decay=0.99)
    b = SoccerBatch(n, 5, 4, 0.2, seed=SEED, autoreset=True)
    mq = b.minimax_q(GAMMA, opponent="self", **kw); ql = b.q_learning(GAMMA, **kw)
    b.reset()
    ck = b.checkpoint()
    mq.run(T)
    b.restore(ck)
    ql.run(T)
    batch = _random_batch(np.random.default_rng(5), b.nS, 3000)
    mq.update(*batch); ql.update(*batch); mq.update(*batch); ql.update(*batch)
    b_m = SoccerBatch(n, 5, 4, 0.2, seed=SEED, autoreset=True)
    mq1 = b_m.minimax_q(GAMMA, opponent="self", **kw)
    b_m.reset(); mq1.run(T); mq1.update(*batch); mq1.update(*batch)
    b_q = SoccerBatch(n, 5, 4, 0.2, seed=SEED, autoreset=True)
    ql1 = b_q.q_learning(GAMMA, **kw)
    b_q.reset(); ql1.run(T); ql1.update(*batch); ql1.update(*batch)
    got, want = mq.read(), mq1.read()
    for k in ("Q", "V", "pi_a", "pi_b", "visits"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert (got["alpha"], got["steps"]) == (want["alpha"], want["steps"])
    assert_learner_equal(ql.read(), ql1.read())
    s1, s2 = b.get_state(), b_q.get_state()                    # (the shared handle's histogram counted both runs)
    for k in s1:
        np.testing.assert_array_equal(s1[k], s2[k])
    assert b.tick == b_q.tick == T + 1
    b.close(); b_m.close(); b_q.close()
    assert mq.q is None and ql.q is None                       # the handle freed both


# ---- 4. refusals ------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=False)
    with pytest.raises(AssertionError, match="SOCCER_F_AUTORESET"):
        b.q_learning(GAMMA)
    b.close()
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=True)
    b.set_policy("player_b", np.zeros(b.nS, np.int8))
    with pytest.raises(AssertionError, match="two-player handle"):
        b.q_learning(GAMMA)
    b.set_policy("player_b", None)
    q = b.q_learning(GAMMA)
    dev = [b.alloc(4, dt).fill(0) for dt in DTYPES]
    b.sync()
    b.graph_begin()
    b.rollout(2, sample_actions=True)           # (something to capture; never replayed)
    for call in (lambda: q.run(1), lambda: q.read(), lambda: q.load(np.zeros((b.nS, 5)), np.zeros((b.nS, 5))),
                 lambda: b.q_learning(GAMMA), lambda: q.update(*dev)):
        with pytest.raises(RuntimeError, match="during graph capture"):
            call()
    b.graph_destroy(b.graph_end())
    other = SoccerBatch(8, 5, 4, 0.0, autoreset=True)
    with pytest.raises(AssertionError, match="not a learner of this handle"):
        other._check(other.lib.soccer_q_learner_run(other.h, q.q, 1))
    other.close()
    # the library's own range checks (the Python layer checks first, so straight through the ABI)
    import ctypes as C
    from gym_soccer_littman94_amd import _lib
    uniform = np.full((b.nS, 5), 0.2)
    bad_row = uniform.copy(); bad_row[3] = [0.5, 0.5, 0.5, 0.0, 0.0]
    negative = uniform.copy(); negative[4] = [1.2, -0.2, 0.0, 0.0, 0.0]
    for fields, msg in ((dict(discount_factor=1.0), "discount_factor"), (dict(alpha=-0.5), "alpha"), (dict(decay=0.0), "decay"),
                        (dict(explor=2.0), "explor"), (dict(q_init=-1.5), "q_init"), (dict(act_a=7), "act_a"), (dict(act_b=-1), "act_b"),
                        (dict(act_a=_lib.QL_FIXED), "policy_a"), (dict(policy_b=uniform.ctypes.data), "policy_b"),
                        (dict(act_a=_lib.QL_FIXED, policy_a=bad_row.ctypes.data), "policy_a\\[3\\] does not sum to 1"),
                        (dict(act_b=_lib.QL_FIXED, policy_b=negative.ctypes.data), "policy_b\\[4\\]\\[1\\] is negative")):
        cfg = _lib.QLearnerConfig(0.9, 1.0, 0.5, 0.2, 1.0, 0, 0, None, None)
        for k, v in fields.items():
            setattr(cfg, k, v)
        out = C.c_void_p()
        assert b.lib.soccer_q_learner_create(b.h, C.byref(cfg), C.byref(out)) == _lib.E_INVALID and not out.value
        assert re.search(msg, b.lib.soccer_last_error(b.h).decode())
    with pytest.raises(AssertionError, match="2\\*\\*22|2\\^22"):
        q.update(np.zeros(2 ** 22 + 1), *[np.zeros(2 ** 22 + 1)] * 5)
    # frozen lanes contribute nothing and raise the flag
    q.run(3)
    assert b.misuse() == SoccerBatch.MISUSE_FROZEN and int(q.read()["visits"].sum()) == 0 and q.steps == 3
    q_other = b.q_learning(GAMMA, act_b="uniform")
    b.close()                                   # with two live learners: the handle frees them
    assert q_other.q is None
    q.close()                                   # the wrapper knows


def test_a_handle_beyond_2_22_lanes_is_refused():
    b = SoccerBatch(2 ** 22 + 4, 5, 4, 0.0, autoreset=True)
    with pytest.raises(AssertionError, match="2\\^22 lanes"):
        b.q_learning(GAMMA)
    b.close()
    b = SoccerBatch(2 ** 22, 5, 4, 0.0, autoreset=True)
    b.reset()
    q = b.q_learning(GAMMA, q_init=1.0)
    q.run(2)                                    # right after a reset every lane sits on an ISD state: the sums' worst case
    r = q.read()
    assert int(r["visits"].sum()) == 2 * 2 ** 22 and max(np.abs(r["Q_a"]).max(), np.abs(r["Q_b"]).max()) <= 1.0
    b.close()


# ---- 5. it learns -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("setup", ["qr", "challenger"])
def test_it_learns_the_best_response_values(setup):
    """5x4, slip 0, gamma 0.9, 65 536 lanes x 3 000 steps from Q = 0, alpha 1 -> 0.01, seed 1994.  QR (greedy A, uniform B): V_a
    against the exact best response to a uniform B.  Challenger (fixed uniform A, greedy B): -V_b against the exact best
    response to a uniform A.  The mean over the live states of the difference is 0.002326 / 0.002559 for the numpy
    restatement with these parameters (tests/test_q_learning_np.py, where the bound comes from), which test 2 pins the
    device to; the maximum (0.0862 / 0.1037 there) is printed, not asserted."""
    n, T = 65536, 3000
    env = VectorSoccerEnv(n, 5, 4, 0.0, seed=1994, autoreset=True)
    uniform = np.full((env.nS, 5), 0.2)
    kw = dict(alpha=1.0, decay=0.01 ** (1.0 / T), explor=0.2, q_init=0.0)
    if setup == "qr":
        want = pl.best_response(env, uniform, 1, 1e-10, GAMMA)[1]
        q = env.q_learning(GAMMA, act_a="greedy", act_b="uniform", **kw)
    else:
        want = pl.best_response(env, uniform, 0, 1e-10, GAMMA)[1]
        q = env.q_learning(GAMMA, act_a=uniform, act_b="greedy", **kw)
    env.reset()
    q.run(T)
    r = q.read()
    err = np.abs((r["V_a"] if setup == "qr" else -r["V_b"]) - want)[1:]
    print("%s: mean %.6f  max %.6f of |V - V(best response)| over live states" % (setup, err.mean(), err.max()))
    assert r["steps"] == T and abs(r["alpha"] - 0.01) < 1e-12
    assert (r["visits"].sum(1)[1:] > 0).all(), "a live state was never visited"
    assert int(r["visits"].sum()) == n * T
    assert err.mean() <= BOUND
    if setup == "qr":
        # the greedy policy plugs into the rollout and into exploitability as it is; the planner-style entry point
        env.rollout(5, sample_actions=True, mixed_policies={"player_a": r["pi_a"], "player_b": r["pi_b"]}, infos="none")
        e = q.exploitability()
        assert e["gap"].shape == (env.nS,) and (e["gap"][1:] >= -1e-9).all()
        env2 = VectorSoccerEnv(4096, 5, 4, 0.0, seed=3, autoreset=True)
        pa, pb, Va, Vb, Qa, Qb, visits = pl.q_learning(env2, 50, GAMMA, q_init=0.0, act_b="uniform")
        assert pa.shape == pb.shape == Qa.shape == Qb.shape == (env2.nS, 5) and Va.shape == Vb.shape == (env2.nS,)
        assert int(visits.sum()) == 4096 * 50 and (pa.sum(1) == 1).all()
        env2.close()
    q.close(); env.close()
