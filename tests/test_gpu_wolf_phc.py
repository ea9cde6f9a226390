"""-m gpu: the policy hill-climbers on the device (include/soccer_hip.h, "learners, policy hill-climbing") against their numpy
restatement (tests/wolf_phc_np.py: the oracle as environment), bit for bit — update() on synthetic batches, run() on four
pitches; then composition and invariance, the Q-learners as a cross-check, the refusals, and the learning test against the
exact best response."""
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
from q_learning_np import behaviour  # noqa: E402
from test_gpu_q_learning import DTYPES, _batches, _random_batch, assert_batches_equal, assert_state_equal  # noqa: E402
from test_wolf_phc_np import (BOUND, GAMMA, LEARN, N_RUN, RUN_CASES, RUN_IDS, RUN_KW, SEED, T_RUN, act, assert_rows_are_policies,  # noqa: E402
                              reference_run)
from wolf_phc_np import WolfPHCNumpy, assert_phc_equal  # noqa: E402

pytestmark = pytest.mark.gpu

ARRAYS = ("Q_a", "Q_b", "pi_a", "pi_b", "avg_a", "avg_b", "visits", "updates")


def checkpoint(r):
    """read()'s dict as load()'s arguments"""
    return dict(Q_a=r["Q_a"], Q_b=r["Q_b"], pi_a=r["pi_a"], pi_b=r["pi_b"], avg_a=r["avg_a"], avg_b=r["avg_b"], visits=r["visits"],
                updates=r["updates"], alpha=r["alpha"], dscale=r["dscale"], steps=r["steps"])


# ---- 1. update() against numpy, exactly ---------------------------------------------------------------
@pytest.mark.parametrize("case", ["random cells", "one row, 65536 samples over all b", "terminated, next_obs 0",
                                  "rewards of both signs in one cell", "n = 1"])
def test_update_equals_numpy_bit_for_bit(case):
    b = SoccerBatch(8, 5, 4, 0.0, seed=1, autoreset=True)
    kw = dict(alpha=0.75, decay=0.9, explor=0.2, q_init=0.5, delta_win=0.1, delta_lose=0.4, delta_decay=0.9)
    q = b.wolf_phc(GAMMA, **kw)
    ref = WolfPHCNumpy(b.nS, GAMMA, **kw)
    assert_phc_equal(q.read(), ref.state())
    warm = _random_batch(np.random.default_rng(7), b.nS, 20000)      # the values leave their initial constant
    for batch in (warm, _batches(b.nS)[case], warm):
        before = q.read()
        q.update(*batch)
        ref.update(*batch)
        got = q.read()
        assert_phc_equal(got, ref.state())
        untouched = np.setdiff1d(np.arange(b.nS), np.unique(batch[0]))
        for k in ARRAYS:
            assert got[k][untouched].tobytes() == before[k][untouched].tobytes(), k
    assert q.steps == 3 and q.alpha == ref.alpha and q.dscale == ref.dscale
    assert ref.n_win > 0 and ref.n_lose > 0
    assert b.misuse() == 0
    dev = [b.alloc(len(x), dt).upload(x) for x, dt in zip(warm, DTYPES)]       # device arrays in
    q.update(*dev); ref.update(*warm)
    assert_phc_equal(q.read(), ref.state())
    q.update(*[np.zeros(0)] * 6); ref.update(*[np.zeros(0, np.int64)] * 6)      # n = 0: alpha, dscale and the counter alone
    assert_phc_equal(q.read(), ref.state())
    assert_rows_are_policies(q.read())
    q.close(); b.close()


def test_update_leaves_bad_transitions_out_and_flags_them():
    b = SoccerBatch(8, 5, 4, 0.0, seed=1, autoreset=True)
    q = b.wolf_phc(GAMMA, q_init=0.25)
    ref = WolfPHCNumpy(b.nS, GAMMA, q_init=0.25)
    good = _random_batch(np.random.default_rng(3), b.nS, 4000)
    bad_act = [x.copy() for x in good]; bad_act[1][::7] = 5; bad_act[2][3::11] = -1
    keep = np.ones(4000, bool); keep[::7] = False; keep[3::11] = False
    q.update(*bad_act); ref.update(*[x[keep] for x in good])
    assert_phc_equal(q.read(), ref.state())
    assert b.misuse() == SoccerBatch.MISUSE_ACTION
    b.reset_stats()
    bad_obs = [x.copy() for x in good]; bad_obs[0][::5] = 0; bad_obs[0][1::9] = b.nS; bad_obs[5][2::13] = b.nS + 3
    keep = np.ones(4000, bool); keep[::5] = False; keep[1::9] = False; keep[2::13] = False
    q.update(*bad_obs); ref.update(*[x[keep] for x in good])
    assert_phc_equal(q.read(), ref.state())
    assert b.misuse() == SoccerBatch.MISUSE_OBSERVATION
    b.reset_stats()
    before = q.read()                   # nothing but bad transitions: alpha, dscale and the step counter move, nothing else does
    q.update(*[np.zeros(10)] * 6)
    after = q.read()
    for k in ARRAYS:
        assert after[k].tobytes() == before[k].tobytes(), k
    assert after["steps"] == before["steps"] + 1 and b.misuse() == SoccerBatch.MISUSE_OBSERVATION
    b.close()


# ---- 2. run(T) against the restatement, exactly --------------------------------------------------------
def _learner(b, act_a, act_b, extra=()):
    kw = dict(RUN_KW); kw.update(dict(extra))
    return b.wolf_phc(GAMMA, act_a=act(act_a, b.nS), act_b=act(act_b, b.nS), **kw)


@pytest.mark.parametrize("case", RUN_CASES, ids=RUN_IDS)
def test_run_equals_the_restatement_bit_for_bit(case):
    w, h, slip, act_a, act_b, extra = case
    o, ref = reference_run(w, h, slip, act_a, act_b, extra)
    assert ref.n_win > 0 and ref.n_lose > 0 and ref.n_clamp > 0
    b = SoccerBatch(N_RUN, w, h, slip, seed=SEED, autoreset=True)
    q = _learner(b, act_a, act_b, extra)
    b.reset()
    q.run(T_RUN)
    assert_phc_equal(q.read(), ref.state())
    assert_state_equal(b, o)
    assert b.tick == o.tick == T_RUN + 1
    hist, misuse = b.stats()
    np.testing.assert_array_equal(hist, o.hist)
    assert misuse == 0 and hist.sum() > 0
    assert q.steps == T_RUN and q.alpha == ref.alpha and q.dscale == ref.dscale
    b.close()


# ---- 3. composition and invariance ----------------------------------------------------------------------
DECAYING = {"delta_decay": 0.98}


def _device_run(parts, w=5, h=4, slip=0.2, act_a="learn", act_b="learn", n=N_RUN, extra=DECAYING):
    b = SoccerBatch(n, w, h, slip, seed=SEED, autoreset=True)
    q = _learner(b, act_a, act_b, extra)
    b.reset()
    for t in parts:
        q.run(t)
    return b, q


def test_runs_compose_and_repeat():
    b1, q1 = _device_run([60]); b2, q2 = _device_run([25, 35]); b3, q3 = _device_run([60])
    r1 = q1.read()
    assert_phc_equal(q2.read(), r1); assert_phc_equal(q3.read(), r1)
    assert_batches_equal(b1, b2); assert_batches_equal(b1, b3)
    assert_phc_equal(r1, reference_run(5, 4, 0.2, "learn", "learn", DECAYING)[1].state())
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
    assert_phc_equal(q2.read(), q1.read())
    assert_batches_equal(b1, b2)
    b1.close(); b2.close()


def test_run_is_rollout_plus_update_step_by_step():
    """run(T) = T x [the 1-step mixed-policy rollout with both players' rows of (1 - explor) pi + explor / 5, recording obs /
    final_obs / reward / terminated, the actions recomputed with the oracle's draw, then update()]"""
    T, n = 12, 4096 + 3
    b1, q1 = _device_run([T], slip=0.0, n=n)
    b2 = SoccerBatch(n, 5, 4, 0.0, seed=SEED, autoreset=True)
    q2 = _learner(b2, "learn", "learn", DECAYING)
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
    assert_phc_equal(q2.read(), q1.read())
    assert_batches_equal(b1, b2)
    b1.close(); b2.close()


def test_read_then_load_on_a_fresh_learner_continues_the_same():
    b1, q1 = _device_run([60])
    b2, q2 = _device_run([25])
    ck = q2.read()
    q3 = _learner(b2, "learn", "learn", DECAYING)                      # a second learner on the same handle
    q3.load(**checkpoint(ck))
    assert_phc_equal(q3.read(), ck)
    q3.run(35)
    assert_phc_equal(q3.read(), q1.read())
    q4 = _learner(b2, "learn", "uniform", DECAYING)                    # without the counts they are zeroed; B does not learn:
    q4.load(ck["Q_a"], ck["Q_b"], pi_a=ck["pi_a"], pi_b=ck["pi_b"])    # its rows are ignored, and avg_a is left as it is
    r4 = q4.read()
    assert r4["Q_a"].tobytes() == ck["Q_a"].tobytes() and r4["Q_b"].tobytes() == ck["Q_b"].tobytes()
    assert r4["pi_a"][1:].tobytes() == ck["pi_a"][1:].tobytes() and (r4["pi_b"] == 0.2).all() and (r4["avg_a"] == 0.2).all()
    assert (r4["visits"] == 0).all() and (r4["updates"] == 0).all() and r4["dscale"] == 1.0
    with pytest.raises(AssertionError, match="\\[-1, 1\\]"):
        q4.load(ck["Q_a"] + 2.0, ck["Q_b"])
    bad = ck["pi_a"].copy(); bad[7] = [0.5, 0.5, 0.5, 0.0, 0.0]
    with pytest.raises(AssertionError, match="soccer_wolf_phc_load: pi_a\\[7\\] does not sum to 1"):
        q4.load(ck["Q_a"], ck["Q_b"], pi_a=bad)
    bad = ck["avg_a"].copy(); bad[9] = [1.25, -0.25, 0.0, 0.0, 0.0]
    with pytest.raises(AssertionError, match="soccer_wolf_phc_load: avg_a\\[9\\]\\[1\\] is negative"):
        q4.load(ck["Q_a"], ck["Q_b"], avg_a=bad)
    q4.load(ck["Q_a"], ck["Q_b"], pi_b=bad)                            # (a player that does not learn: not even checked)
    assert q4.read()["pi_a"].tobytes() == r4["pi_a"].tobytes()         # a refused load changed nothing
    b1.close(); b2.close()


def test_with_both_players_fixed_the_tables_are_a_q_learner_s():
    """the Q side is the Q-learners': on equal handles, with the same two fixed policies, Q_a, Q_b and visits agree bit for bit"""
    T = 40
    b1 = SoccerBatch(N_RUN, 5, 4, 0.2, seed=SEED, autoreset=True)
    b2 = SoccerBatch(N_RUN, 5, 4, 0.2, seed=SEED, autoreset=True)
    pa = np.random.default_rng(11).dirichlet(np.ones(5), b1.nS); pb = np.random.default_rng(12).dirichlet(np.ones(5), b1.nS)
    q1 = b1.wolf_phc(GAMMA, act_a=pa, act_b=pb, **RUN_KW)
    q2 = b2.q_learning(GAMMA, act_a=pa, act_b=pb, explor=RUN_KW["explor"], decay=RUN_KW["decay"])
    b1.reset(); b2.reset()
    q1.run(T); q2.run(T)
    r1, r2 = q1.read(), q2.read()
    for k in ("Q_a", "Q_b", "visits", "V_a", "V_b"):
        assert r1[k].tobytes() == r2[k].tobytes(), k
    assert (r1["alpha"], r1["steps"]) == (r2["alpha"], r2["steps"]) and int(r1["visits"].sum()) == N_RUN * T
    assert r1["pi_a"].tobytes() == pa.tobytes() and r1["avg_b"].tobytes() == pb.tobytes()
    assert ((r1["updates"] > 0) == (r1["visits"].sum(1) > 0)).all()
    assert_batches_equal(b1, b2)
    b1.close(); b2.close()


def test_three_kinds_of_learner_share_a_handle():
    """a minimax-Q learner, a Q-learner and a PHC learner alive on one handle, run one after the other from the same
    checkpoint (state and tick), and their update()s interleaved: each equals its run alone"""
    T, n = 20, 4096 + 3
    kw = dict(explor=0.2, decay=0.99)

    def make(b):
        return (b.minimax_q(GAMMA, opponent="self", **kw), b.q_learning(GAMMA, **kw), _learner(b, "learn", "learn", DECAYING))
    b = SoccerBatch(n, 5, 4, 0.2, seed=SEED, autoreset=True)
    shared = make(b)
    b.reset()
    ck = b.checkpoint()
    batch = _random_batch(np.random.default_rng(5), b.nS, 3000)
    for q in shared:
        b.restore(ck)
        q.run(T)
    for _ in range(2):
        for q in shared:
            q.update(*batch)
    for i in range(3):
        b1 = SoccerBatch(n, 5, 4, 0.2, seed=SEED, autoreset=True)
        alone = make(b1)[i]
        b1.reset(); alone.run(T); alone.update(*batch); alone.update(*batch)
        got, want = shared[i].read(), alone.read()
        assert sorted(got) == sorted(want)
        for k in got:
            assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (i, k)
        assert b.tick == b1.tick == T + 1
        if i == 2:                                             # the shared handle's lanes are where its last run left them
            s1, s2 = b.get_state(), b1.get_state()             # (its histogram counted all three runs)
            for k in s1:
                np.testing.assert_array_equal(s1[k], s2[k])
        b1.close()
    b.close()
    assert all(q.q is None for q in shared)                    # the handle freed all three


# ---- 4. refusals ------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=False)
    with pytest.raises(AssertionError, match="SOCCER_F_AUTORESET"):
        b.wolf_phc(GAMMA)
    b.close()
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=True)
    b.set_policy("player_b", np.zeros(b.nS, np.int8))
    with pytest.raises(AssertionError, match="two-player handle"):
        b.wolf_phc(GAMMA)
    b.set_policy("player_b", None)
    q = b.wolf_phc(GAMMA)
    dev = [b.alloc(4, dt).fill(0) for dt in DTYPES]
    b.sync()
    b.graph_begin()
    b.rollout(2, sample_actions=True)           # (something to capture; never replayed)
    for call in (lambda: q.run(1), lambda: q.read(), lambda: q.load(np.zeros((b.nS, 5)), np.zeros((b.nS, 5))),
                 lambda: b.wolf_phc(GAMMA), lambda: q.update(*dev)):
        with pytest.raises(RuntimeError, match="during graph capture"):
            call()
    b.graph_destroy(b.graph_end())
    other = SoccerBatch(8, 5, 4, 0.0, autoreset=True)
    with pytest.raises(AssertionError, match="not a learner of this handle"):
        other._check(other.lib.soccer_wolf_phc_run(other.h, q.q, 1))
    ql = b.q_learning(GAMMA)                    # another kind of learner of the SAME handle is not one of these either
    with pytest.raises(AssertionError, match="not a learner of this handle"):
        b._check(b.lib.soccer_wolf_phc_run(b.h, ql.q, 1))
    other.close()
    # the library's own range checks (the Python layer checks first, so straight through the ABI)
    uniform = np.full((b.nS, 5), 0.2)
    bad_row = uniform.copy(); bad_row[3] = [0.5, 0.5, 0.5, 0.0, 0.0]
    negative = uniform.copy(); negative[4] = [1.2, -0.2, 0.0, 0.0, 0.0]
    for fields, msg in ((dict(discount_factor=1.0), "discount_factor"), (dict(alpha=-0.5), "alpha"), (dict(decay=0.0), "decay"),
                        (dict(explor=2.0), "explor"), (dict(q_init=-1.5), "q_init"), (dict(delta_win=-0.1), "delta_win"),
                        (dict(delta_lose=1.5), "delta_lose"), (dict(delta_decay=0.0), "delta_decay"), (dict(delta_decay=float("nan")), "delta_decay"),
                        (dict(act_a=7), "act_a"), (dict(act_b=-1), "act_b"),
                        (dict(act_a=_lib.PHC_FIXED), "policy_a"), (dict(policy_b=uniform.ctypes.data), "policy_b"),
                        (dict(act_a=_lib.PHC_FIXED, policy_a=bad_row.ctypes.data), "policy_a\\[3\\] does not sum to 1"),
                        (dict(act_b=_lib.PHC_FIXED, policy_b=negative.ctypes.data), "policy_b\\[4\\]\\[1\\] is negative")):
        cfg = _lib.WolfPHCConfig(0.9, 1.0, 0.5, 0.2, 1.0, 0.01, 0.04, 1.0, 0, 0, None, None)
        for k, v in fields.items():
            setattr(cfg, k, v)
        out = C.c_void_p()
        assert b.lib.soccer_wolf_phc_create(b.h, C.byref(cfg), C.byref(out)) == _lib.E_INVALID and not out.value
        assert re.search(msg, b.lib.soccer_last_error(b.h).decode())
    with pytest.raises(AssertionError, match="2\\*\\*22|2\\^22"):
        q.update(np.zeros(2 ** 22 + 1), *[np.zeros(2 ** 22 + 1)] * 5)
    # frozen lanes contribute nothing and raise the flag
    q.run(3)
    r = q.read()
    assert b.misuse() == SoccerBatch.MISUSE_FROZEN and int(r["visits"].sum()) == 0 and int(r["updates"].sum()) == 0 and q.steps == 3
    q_other = b.wolf_phc(GAMMA, act_b="uniform")
    b.close()                                   # with live learners: the handle frees them
    assert q_other.q is None and ql.q is None
    q.close()                                   # the wrapper knows


def test_a_handle_beyond_2_22_lanes_is_refused():
    b = SoccerBatch(2 ** 22 + 4, 5, 4, 0.0, autoreset=True)
    with pytest.raises(AssertionError, match="2\\^22 lanes"):
        b.wolf_phc(GAMMA)
    b.close()


# ---- 5. it learns, and its policies go where policies go ------------------------------------------------------
def test_it_learns_a_best_response_policy_and_hands_it_over():
    """5x4, slip 0, gamma 0.9, 65 536 lanes x 3 000 steps from Q = 0, alpha 1 -> 0.01, delta_win 0.01, delta_lose 0.04, seed
    1994, player A fixed uniform, player B learning.  pi_b is graded exactly: player A's value of the pair (uniform, pi_b) minus
    that of B's exact best response to uniform, mean over the live states.  0.001213 for the numpy restatement with these
    parameters (tests/test_wolf_phc_np.py, where the bound comes from), which test 2 pins the device to; the maximum (0.0954
    there) and the average policy's lag (0.0122 there) are printed, not asserted."""
    c = LEARN
    n, T = c["n"], c["T"]
    env = VectorSoccerEnv(n, c["width"], c["height"], c["slip"], seed=c["seed"], autoreset=True)
    uniform = np.full((env.nS, 5), 0.2)
    want = pl.best_response(env, uniform, 0, 1e-10, c["gamma"])[1]
    q = env.wolf_phc(c["gamma"], alpha=c["alpha"], decay=0.01 ** (1.0 / T), explor=c["explor"], q_init=c["q_init"],
                     delta_win=c["delta_win"], delta_lose=c["delta_lose"], delta_decay=c["delta_decay"], act_a=uniform, act_b="learn")
    env.reset()
    q.run(T)
    r = q.read()
    V = env._batch.evaluate_policies(uniform, np.stack([r["pi_b"], r["avg_b"]]), 1e-10, c["gamma"])[0]
    d, lag = (V[0] - want)[1:], (V[1] - want)[1:]
    print("pi_b: mean %.6f  max %.6f  min %.3g;  avg_b: mean %.6f;  Q side: mean %.6f" % (
        d.mean(), d.max(), d.min(), lag.mean(), np.abs(-r["V_b"] - want)[1:].mean()))
    assert r["steps"] == T and abs(r["alpha"] - 0.01) < 1e-12 and r["dscale"] == 1.0
    assert (r["visits"].sum(1)[1:] > 0).all(), "a live state was never visited"
    assert int(r["visits"].sum()) == n * T and int(r["updates"].max()) <= T
    assert_rows_are_policies(r)
    assert d.min() >= -1e-9
    assert d.mean() <= BOUND
    # hand-over: the policies and their averages plug into the rollout and into exploitability as they are
    env.rollout(5, sample_actions=True, mixed_policies={"player_a": r["pi_a"], "player_b": r["pi_b"]}, infos="none")
    env.rollout(5, sample_actions=True, mixed_policies={"player_a": r["avg_a"], "player_b": r["avg_b"]}, infos="none")
    for which in ("pi", "avg"):
        e = q.exploitability(which)
        assert e["gap"].shape == (env.nS,) and (e["gap"][1:] >= -1e-9).all()
        e2 = pl.exploitability(env, r[which + "_a"], r[which + "_b"], 1e-10, c["gamma"])
        assert e2["gap"].tobytes() == e["gap"].tobytes()
    with pytest.raises(AssertionError, match="which"):
        q.exploitability("greedy")
    # the planner-style entry point
    env2 = VectorSoccerEnv(4096, 5, 4, 0.0, seed=3, autoreset=True)
    pa, pb, aa, ab, Qa, Qb, visits = pl.wolf_phc(env2, 50, GAMMA, q_init=0.0, delta_win=0.1, delta_lose=0.4, act_b="uniform")
    assert pa.shape == pb.shape == aa.shape == ab.shape == Qa.shape == Qb.shape == (env2.nS, 5)
    assert int(visits.sum()) == 4096 * 50 and (pb == 0.2).all() and (ab == 0.2).all() and (pa[1:] != 0.2).any()
    assert (pa >= 0).all() and np.abs(pa.sum(1) - 1.0).max() < 1e-12
    env2.close()
    q.close(); env.close()
