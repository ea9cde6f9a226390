"""-m gpu: the minimax-Q learner on the device (include/soccer_hip.h, "learners") against its numpy restatement
(tests/minimax_q_np.py: the oracle as environment, the host build of the stage-game solver), bit for bit — update() on
synthetic batches, run() on four pitches; then composition and invariance, the learning test against V* from the
existing minimax value iteration, and the refusals."""
import os
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch, VectorSoccerEnv
from gym_soccer_littman94_amd import planners as pl
from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from minimax_q_np import MinimaxQNumpy, assert_learner_equal, behaviour  # noqa: E402
from test_matrix_game_host import assert_certificate, build_games_host  # noqa: E402

pytestmark = pytest.mark.gpu

GAMMA = 0.9


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_games_host(tmp_path_factory.mktemp("games_mq_gpu"))


def assert_state_equal(b, o):
    s = b.get_state()
    np.testing.assert_array_equal(s["row_a"], o.row_a); np.testing.assert_array_equal(s["col_a"], o.col_a)
    np.testing.assert_array_equal(s["row_b"], o.row_b); np.testing.assert_array_equal(s["col_b"], o.col_b)
    np.testing.assert_array_equal(s["poss"], o.poss & 1)
    np.testing.assert_array_equal(s["needs_reset"], (o.poss >> 1) & 1)
    np.testing.assert_array_equal(s["t"], o.t)


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
        return np.full(n, s), np.full(n, a), np.full(n, b), rew, (rew != 0).astype(np.uint8), np.where(rew != 0, 0, rng.integers(1, nS, n))
    n = 65536
    return {
        "random cells": _random_batch(rng, nS, 5000),
        "one cell, 65536 samples": one(n, 17, 3, 1, np.where(rng.random(n) < 0.1, 1, 0)),
        "terminated, next_obs 0": one(300, 5, 0, 4, np.ones(300, np.int64)),
        "rewards of both signs in one cell": one(1001, nS - 1, 4, 4, rng.choice([-1, 0, 1], 1001)),
        "n = 1": one(1, 9, 2, 2, np.array([-1])),
    }


@pytest.mark.parametrize("case", ["random cells", "one cell, 65536 samples", "terminated, next_obs 0",
                                  "rewards of both signs in one cell", "n = 1"])
def test_update_equals_numpy_bit_for_bit(host, case):
    b = SoccerBatch(8, 5, 4, 0.0, seed=1, autoreset=True)
    kw = dict(alpha=0.75, decay=0.9, explor=0.2, q_init=0.5, opponent="self")
    q = b.minimax_q(GAMMA, **kw)
    ref = MinimaxQNumpy(host, b.nS, GAMMA, **kw)
    assert_learner_equal(q.read(), ref.state())                      # creation: set, not solved
    warm = _random_batch(np.random.default_rng(7), b.nS, 20000)      # V leaves its initial constant
    for batch in (warm, _batches(b.nS)[case], warm):
        before = q.read()
        q.update(*batch)
        ref.update(*batch)
        got = q.read()
        assert_learner_equal(got, ref.state())
        untouched = np.setdiff1d(np.arange(b.nS), np.unique(batch[0]))
        for k in ("Q", "V", "pi_a", "pi_b", "visits"):
            assert got[k][untouched].tobytes() == before[k][untouched].tobytes(), k
    assert q.steps == 3 and q.alpha == ref.alpha
    assert b.misuse() == 0
    # device arrays in, and the properties one by one
    dev = [b.alloc(len(x), dt).upload(x) for x, dt in zip(warm, (np.uint16, np.int8, np.int8, np.int8, np.uint8, np.uint16))]
    q.update(*dev); ref.update(*warm)
    assert_learner_equal(dict(Q=q.Q, V=q.V, pi_a=q.pi_a, pi_b=q.pi_b, visits=q.visits, alpha=q.alpha, steps=q.steps), ref.state())
    q.close(); b.close()


def test_update_leaves_bad_transitions_out_and_flags_them(host):
    b = SoccerBatch(8, 5, 4, 0.0, seed=1, autoreset=True)
    q = b.minimax_q(GAMMA, q_init=0.25)
    ref = MinimaxQNumpy(host, b.nS, GAMMA, q_init=0.25)
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
    # nothing but bad transitions: alpha and the step counter move, nothing else does
    before = q.read()
    q.update(np.zeros(10), np.zeros(10), np.zeros(10), np.zeros(10), np.zeros(10), np.zeros(10))
    after = q.read()
    for k in ("Q", "V", "pi_a", "pi_b", "visits"):
        assert after[k].tobytes() == before[k].tobytes()
    assert after["steps"] == before["steps"] + 1 and b.misuse() == SoccerBatch.MISUSE_OBSERVATION
    b.close()


# ---- 2. run(T) against the restatement, exactly --------------------------------------------------------
N_RUN, T_RUN, SEED = 8192 + 3, 60, 1994
RUN_KW = dict(explor=0.2, decay=0.99)


def _opponent(name, nS):
    if name == "dirichlet":
        return np.random.default_rng(11).dirichlet(np.ones(5), nS)
    return name


def _reference_run(host, w, h, slip, opp, T=T_RUN, n=N_RUN):
    o = Oracle(w, h, slip, n=n, seed=SEED, autoreset=True)
    ref = MinimaxQNumpy(host, o.nS, GAMMA, opponent=_opponent(opp, o.nS), **RUN_KW)
    ref.run(o, o.reset(), T)
    return o, ref


@pytest.mark.parametrize("w,h,slip,opp", [(5, 4, 0.0, "uniform"), (5, 4, 0.2, "self"), (7, 5, 0.3, "dirichlet"), (11, 7, 0.2, "uniform")])
def test_run_equals_the_restatement_bit_for_bit(host, w, h, slip, opp):
    o, ref = _reference_run(host, w, h, slip, opp)
    b = SoccerBatch(N_RUN, w, h, slip, seed=SEED, autoreset=True)
    q = b.minimax_q(GAMMA, opponent=_opponent(opp, b.nS), **RUN_KW)
    b.reset()
    q.run(T_RUN)
    assert_learner_equal(q.read(), ref.state())
    assert_state_equal(b, o)
    assert b.tick == o.tick == T_RUN + 1
    hist, misuse = b.stats()
    np.testing.assert_array_equal(hist, o.hist)
    assert misuse == 0 and hist.sum() > 0
    b.close()


# ---- 3. composition and invariance ----------------------------------------------------------------------
def _device_run(parts, w=5, h=4, slip=0.2, opp="self", n=N_RUN):
    b = SoccerBatch(n, w, h, slip, seed=SEED, autoreset=True)
    q = b.minimax_q(GAMMA, opponent=opp, **RUN_KW)
    b.reset()
    for t in parts:
        q.run(t)
    return b, q


def test_runs_compose_and_repeat(host):
    b1, q1 = _device_run([60]); b2, q2 = _device_run([25, 35]); b3, q3 = _device_run([60])
    r1 = q1.read()
    assert_learner_equal(q2.read(), r1); assert_learner_equal(q3.read(), r1)
    for k in ("row_a", "col_a", "row_b", "col_b", "poss", "t", "needs_reset"):
        np.testing.assert_array_equal(b1.get_state()[k], b2.get_state()[k])
    o, ref = _reference_run(host, 5, 4, 0.2, "self")
    assert_learner_equal(r1, ref.state())
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
    s1, s2 = b1.get_state(), b2.get_state()
    for k in s1:
        np.testing.assert_array_equal(s1[k], s2[k])
    np.testing.assert_array_equal(b1.stats()[0], b2.stats()[0])
    b1.close(); b2.close()


def test_run_is_rollout_plus_update_step_by_step():
    """run(T) = T x [the 1-step mixed-policy rollout recording obs / final_obs / reward / terminated, the actions recomputed
    with the oracle's draw, then update()] — the act kernel is the existing rollout, the update the existing update."""
    T, n = 12, 4096 + 3
    b1, q1 = _device_run([T], slip=0.0, opp="uniform", n=n)
    b2 = SoccerBatch(n, 5, 4, 0.0, seed=SEED, autoreset=True)
    q2 = b2.minimax_q(GAMMA, opponent="uniform", **RUN_KW)
    o = Oracle(5, 4, 0.0, n=n, seed=SEED, autoreset=True)              # its action draw only
    obs_d = b2.alloc(n, np.uint16); fin_d = b2.alloc(n, np.uint16); rew_d = b2.alloc(n, np.int8); term_d = b2.alloc(n, np.uint8)
    mix_d = b2.alloc((b2.nS, 4), np.uint16)
    b2.reset(obs=obs_d)
    obs = obs_d.download()
    for _ in range(T):
        ma = behaviour(q2.pi_a, 0.2)
        mix_d.upload(ma)
        o.tick = b2.tick
        a, bb = o.sample_actions_mixed(obs, ma, None)
        b2.rollout(1, sample_actions=True, mix_a=mix_d, obs=obs_d, reward=rew_d, terminated=term_d, final_obs=fin_d,
                   out_stride=(n + 3) & ~3)        # (a stride the byte-parallel rollout accepts: it takes the step, the per-lane kernel the tail)
        q2.update(obs, a, bb, rew_d.download(), term_d.download(), fin_d.download())
        obs = obs_d.download()
    assert_learner_equal(q2.read(), q1.read())
    s1, s2 = b1.get_state(), b2.get_state()
    for k in s1:
        np.testing.assert_array_equal(s1[k], s2[k])
    assert b1.tick == b2.tick
    np.testing.assert_array_equal(b1.stats()[0], b2.stats()[0])
    b1.close(); b2.close()


def test_read_then_load_on_a_fresh_learner_continues_the_same():
    b1, q1 = _device_run([60])
    b2, q2 = _device_run([25])
    ck = q2.read()
    q3 = b2.minimax_q(GAMMA, opponent="self", **RUN_KW)               # a second learner on the same handle
    q3.load(ck["Q"], visits=ck["visits"], alpha=ck["alpha"], steps=ck["steps"])
    assert_learner_equal(q3.read(), ck)
    q3.run(35)
    assert_learner_equal(q3.read(), q1.read())
    # without the counts every state is solved: the visited ones come out the same
    q4 = b2.minimax_q(GAMMA, opponent="self", **RUN_KW)
    q4.load(ck["Q"])
    seen = ck["visits"].sum(1) > 0
    r4 = q4.read()
    assert r4["V"][seen].tobytes() == ck["V"][seen].tobytes() and r4["pi_a"][seen].tobytes() == ck["pi_a"][seen].tobytes()
    assert (r4["visits"] == 0).all() and (r4["V"][~seen][1:] == 1.0).all()
    b1.close(); b2.close()


# ---- 4. it learns -----------------------------------------------------------------------------------------
def test_it_learns_the_minimax_values():
    """5x4, slip 0, gamma 0.9, 65 536 lanes x 3 000 steps from Q = 0 against a uniform B: max |V - V*| over the live states is
    0.0249 for the numpy restatement with these parameters (tests/test_minimax_q_np.py), which test 2 pins the device to."""
    n, T = 65536, 3000
    env = VectorSoccerEnv(n, 5, 4, 0.0, seed=1994, autoreset=True)
    vstar = pl.minimax_value_iteration(env, 1e-10, GAMMA)[2]
    env.reset()
    q = env.minimax_q(GAMMA, alpha=1.0, decay=0.01 ** (1.0 / T), explor=0.2, q_init=0.0, opponent="uniform")
    q.run(T)
    r = q.read()
    err = np.abs(r["V"] - vstar)[1:].max()
    print("max |V - V*| over live states: %.6f   training episodes (-1, 0, +1): %s" % (err, env.episode_histogram().tolist()))
    assert r["steps"] == T and abs(r["alpha"] - 0.01) < 1e-12
    assert (r["visits"].sum(1)[1:] > 0).all(), "a live state was never visited"
    assert int(r["visits"].sum()) == n * T
    assert_certificate(r["Q"][1:], r["V"][1:], r["pi_a"][1:], r["pi_b"][1:])
    assert err <= 0.07
    # the learned strategy plays: 100 steps against a uniform B
    env.batch.reset_stats()
    env.rollout(100, sample_actions=True, mixed_policies={"player_a": r["pi_a"]}, infos="none")
    hist = env.episode_histogram()
    print("learned pi_a against uniform B, episodes (-1, 0, +1): %s" % hist.tolist())
    assert int(hist[2]) > int(hist[0])
    # and the planner-style entry point returns the same tuple shape
    env2 = VectorSoccerEnv(4096, 5, 4, 0.0, seed=3, autoreset=True)
    pa, pb, V, Q, visits = pl.minimax_q_learning(env2, 50, GAMMA, q_init=0.0)
    assert pa.shape == pb.shape == (env2.nS, 5) and V.shape == (env2.nS,) and Q.shape == (env2.nS, 5, 5)
    assert int(visits.sum()) == 4096 * 50
    env2.rollout(5, sample_actions=True, mixed_policies={"player_a": pa, "player_b": pb})
    q.close(); env.close(); env2.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=False)
    with pytest.raises(AssertionError, match="SOCCER_F_AUTORESET"):
        b.minimax_q(GAMMA)
    b.close()
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=True)
    b.set_policy("player_b", np.zeros(b.nS, np.int8))
    with pytest.raises(AssertionError, match="two-player handle"):
        b.minimax_q(GAMMA)
    b.set_policy("player_b", None)
    q = b.minimax_q(GAMMA)
    dev = [b.alloc(4, dt).fill(0) for dt in (np.uint16, np.int8, np.int8, np.int8, np.uint8, np.uint16)]
    b.sync()
    b.graph_begin()
    b.rollout(2, sample_actions=True)           # (something to capture; never replayed)
    for call in (lambda: q.run(1), lambda: q.read(), lambda: q.load(np.zeros((b.nS, 5, 5))), lambda: b.minimax_q(GAMMA),
                 lambda: q.update(*dev)):
        with pytest.raises(RuntimeError, match="during graph capture"):
            call()
    b.graph_destroy(b.graph_end())
    other = SoccerBatch(8, 5, 4, 0.0, autoreset=True)
    with pytest.raises(AssertionError, match="not a learner of this handle"):
        other._check(other.lib.soccer_minimax_q_run(other.h, q.q, 1))
    other.close()
    # the library's own range checks (the Python layer checks first, so straight through the ABI)
    import ctypes as C
    from gym_soccer_littman94_amd import _lib
    for field, value, msg in (("discount_factor", 1.0, "discount_factor"), ("alpha", -0.5, "alpha"), ("decay", 0.0, "decay"),
                              ("explor", 2.0, "explor"), ("q_init", -1.5, "q_init"), ("opponent", 7, "opponent")):
        cfg = _lib.MinimaxQConfig(0.9, 1.0, 0.5, 0.2, 1.0, 0, 0, None)
        setattr(cfg, field, value)
        out = C.c_void_p()
        assert b.lib.soccer_minimax_q_create(b.h, C.byref(cfg), C.byref(out)) == _lib.E_INVALID and not out.value
        assert msg in b.lib.soccer_last_error(b.h).decode()
    with pytest.raises(AssertionError, match="2\\*\\*22|2\\^22"):
        q.update(np.zeros(2 ** 22 + 1), *[np.zeros(2 ** 22 + 1)] * 5)
    # frozen lanes contribute nothing and raise the flag
    q.run(3)
    assert b.misuse() == SoccerBatch.MISUSE_FROZEN and int(q.visits.sum()) == 0 and q.steps == 3
    q_other = b.minimax_q(GAMMA, opponent="self")
    b.close()                                   # with two live learners: the handle frees them
    assert q_other.q is None
    q.close()                                   # the wrapper knows


def test_a_handle_beyond_2_22_lanes_is_refused():
    b = SoccerBatch(2 ** 22 + 4, 5, 4, 0.0, autoreset=True)
    with pytest.raises(AssertionError, match="2\\^22 lanes"):
        b.minimax_q(GAMMA)
    b.close()
    b = SoccerBatch(2 ** 22, 5, 4, 0.0, autoreset=True)
    b.reset()
    q = b.minimax_q(GAMMA, q_init=1.0)
    q.run(2)                                    # right after a reset every lane sits on an ISD state: the sums' worst case
    r = q.read()
    assert int(r["visits"].sum()) == 2 * 2 ** 22 and np.abs(r["Q"]).max() <= 1.0
    b.close()
