"""-m gpu: the regret matchers of one table on the device (include/soccer_hip.h, "learners, regret matching") against their
numpy restatement (tests/regret_matching_np.py: the oracle as environment), bit for bit — update() on synthetic batches, run()
on five cases; then composition and invariance, checkpoints, the refusals, sharing a handle, exploitability, and the learning
run.  Every comparison is to the bits of Q, R, Z, visits, updates, alpha and steps, plus lane state, tick and histogram."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch, VectorSoccerEnv, _lib
from gym_soccer_littman94_amd import planners as pl
from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from q_learning_np import behaviour  # noqa: E402
from regret_matching_np import ROWS, RegretMatchingNumpy, assert_regret_equal  # noqa: E402
from test_gpu_q_learning import DTYPES, _batches, _random_batch, assert_batches_equal, assert_state_equal  # noqa: E402
from test_regret_matching_np import GAMMA, LEARN, N_RUN, RUN_CASES, RUN_IDS, RUN_KW, SEED, T_RUN, act, learning_run, reference_run  # noqa: E402

pytestmark = pytest.mark.gpu

ARRAYS = ROWS + ("visits", "updates")
FLAGS = [(True, False), (True, True), (False, False), (False, True)]


def checkpoint(r):
    """read()'s dict as load()'s arguments"""
    return {k: r[k] for k in ARRAYS + ("alpha", "steps")}


def assert_derived(r, ref):
    for k, want in ref.derived().items():
        assert r[k].tobytes() == want.tobytes(), k


# ---- 1. update() against numpy, exactly ---------------------------------------------------------------
@pytest.mark.parametrize("plus,linear", FLAGS, ids=["plus", "plus linear", "plain", "plain linear"])
def test_update_equals_numpy_bit_for_bit(plus, linear):
    b = SoccerBatch(8, 5, 4, 0.0, seed=1, autoreset=True)
    kw = dict(alpha=0.75, decay=0.9, explor=0.2, q_init=0.5, plus=plus, linear=linear)
    q = b.regret_matching(GAMMA, **kw)
    ref = RegretMatchingNumpy(b.nS, GAMMA, **kw)
    assert_regret_equal(q.read(), ref.state())
    warm = _random_batch(np.random.default_rng(7), b.nS, 20000)      # the values leave their initial constant
    cases = _batches(b.nS)
    assert len(cases) == 5
    for batch in [warm] + [cases[k] for k in cases] + [warm]:
        before = q.read()
        q.update(*batch)
        ref.update(*batch)
        got = q.read()
        assert_regret_equal(got, ref.state())
        untouched = np.setdiff1d(np.arange(b.nS), np.unique(batch[0]))
        for k in ARRAYS:
            assert got[k][untouched].tobytes() == before[k][untouched].tobytes(), k
    assert q.steps == 7 and q.alpha == ref.alpha
    assert ref.n_fallback > 0 and (ref.n_floor > 0 if plus else ref.n_negative > 0)
    assert b.misuse() == 0
    dev = [b.alloc(len(x), dt).upload(x) for x, dt in zip(warm, DTYPES)]       # device arrays in
    q.update(*dev); ref.update(*warm)
    assert_regret_equal(q.read(), ref.state())
    before = q.read()
    q.update(*[np.zeros(0)] * 6); ref.update(*[np.zeros(0, np.int64)] * 6)      # n = 0: alpha and the counter alone
    after = q.read()
    assert_regret_equal(after, ref.state())
    for k in ARRAYS:
        assert after[k].tobytes() == before[k].tobytes(), k
    assert after["steps"] == before["steps"] + 1 and after["alpha"] == before["alpha"] * 0.9
    assert_derived(after, ref)
    q.close(); b.close()


def test_update_leaves_bad_transitions_out_and_flags_them():
    b = SoccerBatch(8, 5, 4, 0.0, seed=1, autoreset=True)
    q = b.regret_matching(GAMMA, q_init=0.25)
    ref = RegretMatchingNumpy(b.nS, GAMMA, q_init=0.25)
    good = _random_batch(np.random.default_rng(3), b.nS, 4000)
    bad_act = [x.copy() for x in good]; bad_act[1][::7] = 5; bad_act[2][3::11] = -1
    keep = np.ones(4000, bool); keep[::7] = False; keep[3::11] = False
    q.update(*bad_act); ref.update(*[x[keep] for x in good])
    assert_regret_equal(q.read(), ref.state())
    assert b.misuse() == SoccerBatch.MISUSE_ACTION
    b.reset_stats()
    bad_obs = [x.copy() for x in good]; bad_obs[0][::5] = 0; bad_obs[0][1::9] = b.nS; bad_obs[5][2::13] = b.nS + 3
    keep = np.ones(4000, bool); keep[::5] = False; keep[1::9] = False; keep[2::13] = False
    q.update(*bad_obs); ref.update(*[x[keep] for x in good])
    assert_regret_equal(q.read(), ref.state())
    assert b.misuse() == SoccerBatch.MISUSE_OBSERVATION
    b.reset_stats()
    before = q.read()                   # nothing but bad transitions: alpha and the step counter move, nothing else does
    q.update(*[np.zeros(10)] * 6)
    after = q.read()
    for k in ARRAYS:
        assert after[k].tobytes() == before[k].tobytes(), k
    assert after["steps"] == before["steps"] + 1 and b.misuse() == SoccerBatch.MISUSE_OBSERVATION
    b.close()


# ---- 2. run(T) against the restatement, exactly --------------------------------------------------------
def _learner(b, act_a, act_b, plus, linear, **kw):
    return b.regret_matching(GAMMA, act_a=act(act_a, b.nS), act_b=act(act_b, b.nS), plus=plus, linear=linear, **dict(RUN_KW, **kw))


@pytest.mark.parametrize("case", RUN_CASES, ids=RUN_IDS)
def test_run_equals_the_restatement_bit_for_bit(case):
    w, h, slip, act_a, act_b, plus, linear, max_steps = case
    o, ref = reference_run(*case)
    b = SoccerBatch(N_RUN, w, h, slip, seed=SEED, autoreset=True, max_steps=max_steps)
    q = _learner(b, act_a, act_b, plus, linear)
    b.reset()
    q.run(T_RUN)
    r = q.read()
    assert_regret_equal(r, ref.state())
    assert_derived(r, ref)
    assert_state_equal(b, o)
    assert b.tick == o.tick == T_RUN + 1
    hist, misuse = b.stats()
    np.testing.assert_array_equal(hist, o.hist)
    assert misuse == 0 and hist.sum() > 0
    assert q.steps == T_RUN and q.alpha == ref.alpha
    if max_steps == 5:
        assert ref.n_truncated > ref.n_terminated > 0
    b.close()


# ---- 3. composition and invariance ----------------------------------------------------------------------
PLAIN_LINEAR = RUN_CASES[1]             # 5x4 slip 0.2, learn / learn, plain, linear


def _device_run(parts, slip=0.2, n=N_RUN, plus=False, linear=True):
    b = SoccerBatch(n, 5, 4, slip, seed=SEED, autoreset=True)
    q = _learner(b, "learn", "learn", plus, linear)
    b.reset()
    for t in parts:
        q.run(t)
    return b, q


def test_runs_compose():
    b1, q1 = _device_run([60]); b2, q2 = _device_run([25, 35])
    r1 = q1.read()
    assert_regret_equal(q2.read(), r1)
    assert_batches_equal(b1, b2)
    assert_regret_equal(r1, reference_run(*PLAIN_LINEAR)[1].state())
    b1.close(); b2.close()


@pytest.mark.parametrize("var,value", [("SOCCER_SWAR_LAUNCH_LANES", "4096"), ("SOCCER_STATE_LAYOUT", "wide")])
def test_result_does_not_depend_on_launch_split_or_state_layout(var, value, monkeypatch):
    monkeypatch.setenv(var, value)
    b2, q2 = _device_run([60])
    monkeypatch.delenv(var)
    if var == "SOCCER_STATE_LAYOUT":
        assert b2.state_streams() == 6
    o, ref = reference_run(*PLAIN_LINEAR)
    assert_regret_equal(q2.read(), ref.state())
    assert_state_equal(b2, o)
    b2.close()


def test_run_is_rollout_plus_update_step_by_step():
    """run(T) = T x [the 1-step mixed-policy rollout with both players' rows of (1 - explor) pi + explor / 5, recording obs /
    final_obs / reward / terminated, the actions recomputed with the oracle's draw, then update()]"""
    T, n = 12, 4096 + 3
    b1, q1 = _device_run([T], slip=0.0, n=n)
    b2 = SoccerBatch(n, 5, 4, 0.0, seed=SEED, autoreset=True)
    q2 = _learner(b2, "learn", "learn", False, True)
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
    assert_regret_equal(q2.read(), q1.read())
    assert_batches_equal(b1, b2)
    b1.close(); b2.close()


def test_read_then_load_on_a_fresh_learner_continues_the_same_and_refused_loads_write_nothing():
    b2, q2 = _device_run([25], plus=True, linear=False)
    ck = q2.read()
    q3 = _learner(b2, "learn", "learn", True, False)                   # a second learner on the same handle
    q3.load(**checkpoint(ck))
    assert_regret_equal(q3.read(), ck)
    state = b2.checkpoint()
    q2.run(35)
    want = q2.read()
    b2.restore(state)
    q3.run(35)
    assert_regret_equal(q3.read(), want)
    # without the counts they are zeroed; B does not learn: its arrays are ignored, and Z_a is left as it is
    q4 = _learner(b2, "learn", "uniform", True, False)
    nan = np.full((b2.nS, 5), np.nan)
    q4.load(ck["Q_a"], ck["Q_b"], R_a=ck["R_a"], R_b=nan, Z_b=nan)
    r4 = q4.read()
    assert r4["Q_a"].tobytes() == ck["Q_a"].tobytes() and r4["Q_b"].tobytes() == ck["Q_b"].tobytes()
    assert r4["R_a"].tobytes() == ck["R_a"].tobytes() and (r4["Z_a"] == 0.0).all() and (r4["R_b"] == 0.0).all() and (r4["Z_b"] == 0.0).all()
    assert (r4["visits"] == 0).all() and (r4["updates"] == 0).all() and (r4["pi_b"] == 0.2).all()
    # the refused loads name array, state and action, and write nothing
    bad = ck["R_a"].copy(); bad[7, 3] = -0.125
    with pytest.raises(AssertionError, match="soccer_regret_learner_load: R_a\\[7\\]\\[3\\] is negative or not a finite number"):
        q4.load(ck["Q_a"], ck["Q_b"], R_a=bad)
    bad = ck["Z_a"].copy(); bad[9, 1] = np.nan
    with pytest.raises(AssertionError, match="soccer_regret_learner_load: Z_a\\[9\\]\\[1\\] is negative or not a finite number"):
        q4.load(ck["Q_a"] * 0.5, ck["Q_b"], Z_a=bad)
    bad = ck["Q_b"].copy(); bad[5, 2] = 1.5
    with pytest.raises(AssertionError, match="\\[-1, 1\\]"):
        q4.load(ck["Q_a"] * 0.5, bad)
    with pytest.raises(AssertionError, match="soccer_regret_learner_load: Q_b\\[5\\]\\[2\\] is outside \\[-1, 1\\]"):
        q4._call("_load", (), dict(Q_a=ck["Q_a"] * 0.5, Q_b=bad), None)      # (the Python layer checks first: straight to the library)
    with pytest.raises(AssertionError, match="alpha"):
        q4.load(ck["Q_a"], ck["Q_b"], alpha=1.5)
    after = q4.read()
    for k in ARRAYS + ("alpha", "steps"):
        assert np.asarray(after[k]).tobytes() == np.asarray(r4[k]).tobytes(), k
    # a plain learner takes negative regrets, and an infinite one is refused
    q5 = _learner(b2, "learn", "learn", False, False)
    neg = ck["R_a"] - 1.0
    q5.load(ck["Q_a"], ck["Q_b"], R_a=neg)
    assert q5.read()["R_a"][1:].tobytes() == neg[1:].tobytes() and (q5.read()["R_a"][0] == 0.0).all()      # row 0 is taken as zeros
    bad = neg.copy(); bad[3, 0] = -np.inf
    with pytest.raises(AssertionError, match="soccer_regret_learner_load: R_a\\[3\\]\\[0\\] is not a finite number"):
        q5.load(ck["Q_a"], ck["Q_b"], R_a=bad)
    b2.close()


# ---- 4. refusals ------------------------------------------------------------------------------------------
def test_refused_creations_name_their_reason_and_cost_no_tick():
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=True)
    b.reset()
    tick = b.tick
    b.set_policy("player_b", np.zeros(b.nS, np.int8))
    with pytest.raises(AssertionError, match="two-player handle"):                 # a single-agent handle
        b.regret_matching(GAMMA)
    b.set_policy("player_b", None)
    bad_row = np.full((b.nS, 5), 0.2); bad_row[3] = [0.5, 0.5, 0.5, 0.0, 0.0]
    with pytest.raises(AssertionError, match="state 3"):                           # the Python layer's check
        b.regret_matching(GAMMA, act_a=bad_row)
    for fields, msg in ((dict(act_a=_lib.PHC_FIXED, policy_a=bad_row.ctypes.data), "policy_a[3] does not sum to 1"),
                        (dict(plus=2), "plus / linear"), (dict(act_b=7), "act_a / act_b"), (dict(explor=2.0), "explor"),
                        (dict(policy_b=bad_row.ctypes.data), "policy_b goes with")):
        cfg = _lib.RegretLearnerConfig(0.9, 1.0, 0.5, 0.2, 1.0, 0, 0, 1, 0, None, None)
        for k, v in fields.items():
            setattr(cfg, k, v)
        out = C.c_void_p()
        assert b.lib.soccer_regret_learner_create(b.h, C.byref(cfg), C.byref(out)) == _lib.E_INVALID and not out.value
        assert msg in b.lib.soccer_last_error(b.h).decode()
    q = b.regret_matching(GAMMA)
    dev = [b.alloc(4, dt).fill(0) for dt in DTYPES]
    b.sync()
    assert b.tick == tick                       # no refusal so far cost a tick, nor did a creation
    b.graph_begin()
    b.rollout(2, sample_actions=True)           # (something to capture; never replayed)
    tick = b.tick
    for call in (lambda: b.regret_matching(GAMMA), lambda: q.run(1), lambda: q.read(),
                 lambda: q.load(np.zeros((b.nS, 5)), np.zeros((b.nS, 5))), lambda: q.update(*dev)):
        with pytest.raises(RuntimeError, match="during graph capture"):
            call()
    assert b.tick == tick                       # nor one during the capture
    b.graph_destroy(b.graph_end())
    wolf = b.wolf_phc(GAMMA)                    # another kind of learner of the SAME handle is not one of these
    with pytest.raises(AssertionError, match="not a learner of this handle"):
        b._check(b.lib.soccer_regret_learner_run(b.h, wolf.q, 1))
    with pytest.raises(AssertionError, match="2\\*\\*22|2\\^22"):
        q.update(np.zeros(2 ** 22 + 1), *[np.zeros(2 ** 22 + 1)] * 5)
    q.run(2)                                    # after the refusals the learner works
    assert q.steps == 2 and int(q.read()["visits"].sum()) == 2 * 64
    b.close()
    assert q.q is None and wolf.q is None       # the handle freed them
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=False)
    with pytest.raises(AssertionError, match="SOCCER_F_AUTORESET"):
        b.regret_matching(GAMMA)
    b.close()


def test_a_handle_beyond_2_22_lanes_is_refused():
    b = SoccerBatch(2 ** 22 + 4, 5, 4, 0.0, autoreset=True)
    tick = b.tick
    with pytest.raises(AssertionError, match="2\\^22 lanes"):
        b.regret_matching(GAMMA)
    assert b.tick == tick
    b.close()


# ---- 5. sharing a handle ------------------------------------------------------------------------------------
def test_this_learner_a_wolf_phc_and_a_regret_population_share_a_handle():
    """alive on one handle, run one after the other from the same checkpoint (state and tick): each equals its run alone"""
    T, n = 20, 2048 + 3
    kw = dict(explor=0.2, decay=0.99)

    def make(b):
        return (b.regret_matching(GAMMA, **kw), b.wolf_phc(GAMMA, delta_win=0.1, delta_lose=0.4, **kw), b.regret_population(GAMMA, **kw))
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


# ---- 6. it learns, and its policies go where policies go ------------------------------------------------------
def test_the_learning_run_equals_the_restatement_and_its_policies_are_evaluated():
    """The learning run of tests/test_regret_matching_np.py (5x4, slip 0, 8 192 lanes x 500 steps of self-play from Q = 0,
    regret matching+) on the device, to the bits; so the average pair's exact gap is the restatement's, strictly below the
    uniform pair's, which is asserted here again with the device's own evaluator."""
    c = LEARN
    o, ref = learning_run()
    env = VectorSoccerEnv(c["n"], c["width"], c["height"], c["slip"], seed=c["seed"], autoreset=True)
    q = env.regret_matching(c["gamma"], alpha=c["alpha"], decay=0.01 ** (1.0 / c["T"]), explor=c["explor"], q_init=c["q_init"],
                            plus=c["plus"], linear=c["linear"])
    env.reset()
    q.run(c["T"])
    r = q.read()
    assert_regret_equal(r, ref.state())
    assert_derived(r, ref)
    assert_state_equal(env._batch, o)
    uniform = np.full((env.nS, 5), 0.2)
    gaps = {}
    for which in ("avg", "pi"):
        e = q.exploitability(which)
        assert e["gap"].shape == (env.nS,) and (e["gap"][1:] >= -1e-9).all()
        e2 = pl.exploitability(env, r[which + "_a"], r[which + "_b"], 1e-10, c["gamma"])
        assert e2["gap"].tobytes() == e["gap"].tobytes()
        gaps[which] = float(e["gap"][1:].mean())
    g_uniform = float(pl.exploitability(env, uniform, uniform, 1e-10, c["gamma"])["gap"][1:].mean())
    print("mean exact gap over the live states: uniform pair %.4f, average pair %.4f, current pair %.4f" % (g_uniform, gaps["avg"], gaps["pi"]))
    assert gaps["avg"] < g_uniform
    with pytest.raises(AssertionError, match="which"):
        q.exploitability("greedy")
    # hand-over: the policies plug into the rollout as they are; and the planner-style entry point
    env.rollout(5, sample_actions=True, mixed_policies={"player_a": r["avg_a"], "player_b": r["avg_b"]}, infos="none")
    env2 = VectorSoccerEnv(4096, 5, 4, 0.0, seed=3, autoreset=True)
    aa, ab, pa, pb, Qa, Qb, visits = pl.regret_matching(env2, 50, GAMMA, q_init=0.0, act_b="uniform")
    assert pa.shape == pb.shape == aa.shape == ab.shape == Qa.shape == Qb.shape == (env2.nS, 5)
    assert int(visits.sum()) == 4096 * 50 and (pb == 0.2).all() and (ab == 0.2).all() and (aa[1:] != 0.2).any()
    assert (aa >= 0).all() and np.abs(aa.sum(1) - 1.0).max() < 1e-12
    env2.close()
    q.close(); env.close()
