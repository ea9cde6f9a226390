"""-m gpu: the population of opponent-modelling Q-learners, a learner per lane (include/soccer_hip.h, "learners, a population
of opponent-modelling Q-learners") against its numpy restatement (tests/om_population_np.py: the oracle as environment), bit
for bit in Q_a, Q_b, C_a, C_b, alpha and steps — update() on chosen transitions, run() on six shapes; then launch boundaries,
per-member hyperparameters, invariance and round trips, frozen lanes, the derived values and the exact scores, the refusals,
and the learning run against the exact best response.  Conventions of tests/test_gpu_q_population.py: its seed, its T."""
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
from large_pitch_cases import CASES as PITCHES  # noqa: E402
from om_population_np import OMPopulationNumpy, assert_om_population_equal, derive  # noqa: E402
from test_om_population_np import BOUND, LEARN  # noqa: E402
from test_population_edges_np import CASES as EDGE_CASES, KW as EDGE_KW, reference_g0  # noqa: E402

G0 = EDGE_CASES["G0"]

pytestmark = pytest.mark.gpu

GAMMA = 0.9
DTYPES = (np.uint16, np.int8, np.int8, np.int8, np.uint8, np.uint16)
SEED, T_RUN = 1994, 60
RUN_KW = dict(explor=0.2, decay=0.99)
KEYS = ("Q_a", "Q_b", "C_a", "C_b", "alpha")


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
    kw = dict(alpha=0.75, decay=0.9, explor=0.2, q_init=0.5)
    q = b.om_population(GAMMA, **kw)
    ref = OMPopulationNumpy(n, nS, GAMMA, **kw)
    assert_om_population_equal(q.read(), ref.state())
    rng = np.random.default_rng(1994)
    warm = _valid(rng, nS, n)
    warm[0][3] = 40; warm[1][3] = 1; warm[2][3] = 2; warm[3][3] = 1; warm[4][3] = 1; warm[5][3] = 0    # member 3: its row 40 rises now (a goal) ...
    case = _valid(rng, nS, n)

    def put(i, s, a, bb, r, term, s2):
        for k, v in enumerate((s, a, bb, r, term, s2)):
            case[k][i] = v
    put(0, 17, 2, 0, 0, 0, 17)          # s' == s: the bootstrap is the value before the update
    put(1, 5, 0, 4, 1, 1, 0)            # terminated, next_obs 0, r = +1
    put(2, 5, 4, 4, -1, 1, 0)           # r = -1
    put(3, 77, 3, 3, 0, 0, 40)          # ... and is what this transition bootstraps from
    put(4, 17, 1, 1, 1, 1, 300)         # terminated with a live next_obs: still no bootstrap
    put(5, int(warm[0][5]), int(warm[1][5]), int(warm[2][5]), 0, 0, 9)       # a repeated (s, a, b)
    bad_act, bad_obs = [10, 11, 12], [20, 21, 22]
    case[1][10] = 5; case[2][11] = -1; case[1][12] = 100
    case[0][20] = 0; case[0][21] = nS; case[5][22] = nS + 3
    keep = np.ones(n, bool); keep[bad_act + bad_obs] = False
    for batch, kp, flags in ((warm, None, 0), (case, keep, SoccerBatch.MISUSE_ACTION | SoccerBatch.MISUSE_OBSERVATION), (warm, None, 0)):
        before = q.read()
        first_seen = ref.n_first_seen
        q.update(*batch)
        ref.update(*batch, keep=kp)
        got = q.read()
        assert_om_population_equal(got, ref.state())
        assert b.misuse() == flags
        b.reset_stats()
        if kp is not None:
            for i in bad_act + bad_obs:             # flag raised, that member's tables and counts unchanged, alpha advanced
                assert all(got[k][i].tobytes() == before[k][i].tobytes() for k in KEYS[:4])
                assert got["alpha"][i] == before["alpha"][i] * 0.9
            # member 3: the warm update scored at (40, 1, 2), so A at 40 now answers what it saw, a B that plays 2
            assert got["Q_a"][3, 40, 1, 2] == 0.875 and before["V_a"][3, 40] == 0.875 and before["pi_a"][3, 40, 1] == 1.0
            assert got["Q_a"][3, 77, 3, 3] == 0.5 + before["alpha"][3] * (0.9 * 0.875 - 0.5)
            assert got["C_a"][5, warm[0][5], warm[2][5]] == 2 and got["C_b"][5, warm[0][5], warm[1][5]] == 2      # the repeated cell
            assert 0 < ref.n_first_seen - first_seen < keep.sum()     # first-seen states, and states seen before
        moved = (got["Q_a"] != before["Q_a"]).sum((1, 2, 3))
        assert (moved <= 1).all() and all((got[k][:, 0] == 0).all() for k in KEYS[:4])
        np.testing.assert_array_equal(got["C_a"].sum(2), got["C_b"].sum(2))
    assert q.steps == 3 and (q.alpha == ref.alpha).all()
    dev = [b.alloc(n, dt).upload(np.ascontiguousarray(x, dt)) for x, dt in zip(warm, DTYPES)]       # device arrays in
    q.update(*dev); ref.update(*warm)
    assert_om_population_equal(q.read(), ref.state())
    with pytest.raises(AssertionError, match="one transition per member"):
        q.update(*[x[:5] for x in warm])
    q.close(); b.close()


# ---- 2. run(T) against the restatement, exactly --------------------------------------------------------
def _act(name, nS):
    if name == "dirichlet":
        return np.random.default_rng(11).dirichlet(np.ones(5), nS)
    return name


_REFERENCE = {}


def _reference_run(w, h, slip, act_a, act_b, n, max_steps=100, T=T_RUN, kw=None, reset=True):
    """computed once per case and left unchanged"""
    key = (w, h, slip, act_a, act_b, n, max_steps, T, reset, None if kw is None else id(kw))
    if key not in _REFERENCE:
        o = Oracle(w, h, slip, n=n, seed=SEED, autoreset=True, max_steps=max_steps)
        ref = OMPopulationNumpy(n, o.nS, GAMMA, act_a=_act(act_a, o.nS), act_b=_act(act_b, o.nS), **(RUN_KW if kw is None else kw))
        ref.run(o, o.reset(), T)
        _REFERENCE[key] = (o, ref)
    return _REFERENCE[key]


def _device_run(parts, w=5, h=4, slip=0.2, act_a="greedy", act_b="greedy", n=259, max_steps=5, kw=None, reset=True):
    b = SoccerBatch(n, w, h, slip, seed=SEED, autoreset=True, max_steps=max_steps)
    q = b.om_population(GAMMA, act_a=_act(act_a, b.nS), act_b=_act(act_b, b.nS), **(RUN_KW if kw is None else kw))
    if reset:
        b.reset()
    for t in parts:
        q.run(t)
    return b, q


RUN_CASES = [(5, 4, 0.0, "greedy", "uniform", 1, 100), (5, 4, 0.0, "greedy", "uniform", 67, 100), (5, 4, 0.2, "greedy", "greedy", 259, 5),
             (7, 5, 0.3, "dirichlet", "greedy", 67, 100), (11, 7, 0.2, "uniform", "greedy", 67, 100),
             # 12x14: om_pop_run_kernel with the observation table in global memory
             (12, 14, 0.2, "greedy", "greedy", 17, 100)]


@pytest.mark.parametrize("w,h,slip,act_a,act_b,n,max_steps", RUN_CASES)
def test_run_equals_the_restatement_bit_for_bit(w, h, slip, act_a, act_b, n, max_steps):
    o, ref = _reference_run(w, h, slip, act_a, act_b, n, max_steps)
    b, q = _device_run([T_RUN], w, h, slip, act_a, act_b, n, max_steps)
    if (w, h) == (12, 14):
        assert not PITCHES["12x14"]["lut_lds"]      # the observation table does not fit the LDS line: LUT_LDS is false
    assert_om_population_equal(q.read(), ref.state())
    assert_state_equal(b, o)
    assert b.tick == o.tick == T_RUN + 1
    hist, misuse = b.stats()
    np.testing.assert_array_equal(hist, o.hist)
    assert misuse == 0 and ref.n_left_out == 0
    assert q.steps == T_RUN and (q.alpha == ref.alpha).all()
    if n > 1:
        assert ref.n_same > 0 and ref.n_first_seen > 0
    if max_steps == 5:
        assert ref.n_truncated_only > 0 and ref.n_terminated > 0 and ref.n_same > 0 and ref.n_first_seen > 0 and hist.sum() > 0
    part = q.read(n // 2, 1)                       # a range is the slice
    assert part["Q_a"].tobytes() == ref.Q_a[n // 2:n // 2 + 1].tobytes() and part["alpha"][0] == ref.alpha[n // 2]
    assert part["C_b"].tobytes() == ref.C_b[n // 2:n // 2 + 1].tobytes()
    b.close()


def test_run_on_12x14_without_slip_equals_the_restatement_bit_for_bit():
    """case G0 of tests/test_population_edges_np.py, which shows without a GPU that it terminates, truncates and meets s' == s:
    om_pop_run_kernel<SLIP = false, LUT_LDS = false>"""
    c = G0
    o, ref = reference_g0("om")
    assert (c["w"], c["h"], c["slip"]) == (12, 14, 0.0) and not PITCHES["12x14"]["lut_lds"] and RUN_KW == EDGE_KW["q"]
    b, q = _device_run([c["T"]], c["w"], c["h"], c["slip"], "greedy", "greedy", c["n"], c["max_steps"])
    assert_om_population_equal(q.read(), ref.state())
    assert_state_equal(b, o)
    assert b.tick == o.tick == c["T"] + 1
    hist, misuse = b.stats()
    np.testing.assert_array_equal(hist, o.hist)
    assert misuse == 0 and ref.n_left_out == 0
    assert q.steps == c["T"] and (q.alpha == ref.alpha).all()
    assert ref.n_truncated_only > 0 and ref.n_terminated > 0 and ref.n_same > 0 and ref.n_first_seen > 0 and hist.sum() > 0
    b.close()


# ---- 3. launch boundaries --------------------------------------------------------------------------------
def test_runs_compose():
    b1, q1 = _device_run([60]); b2, q2 = _device_run([25, 35])
    assert_om_population_equal(q2.read(), q1.read())
    assert_batches_equal(b1, b2)
    assert_om_population_equal(q1.read(), _reference_run(5, 4, 0.2, "greedy", "greedy", 259, 5)[1].state())
    b1.close(); b2.close()


def test_result_does_not_depend_on_the_steps_per_launch(monkeypatch):
    """slip 0: a Philox block spans eight ticks, so with seven steps per launch a launch starts in the middle of a block"""
    args = dict(slip=0.0, act_b="uniform", n=67, max_steps=100)
    b1, q1 = _device_run([60], **args)
    monkeypatch.setenv("SOCCER_POP_LAUNCH_STEPS", "7")
    b2, q2 = _device_run([60], **args)
    monkeypatch.delenv("SOCCER_POP_LAUNCH_STEPS")
    assert_om_population_equal(q2.read(), q1.read())
    assert_batches_equal(b1, b2)
    assert_om_population_equal(q1.read(), _reference_run(5, 4, 0.0, "greedy", "uniform", 67)[1].state())
    b1.close(); b2.close()


def test_result_does_not_depend_on_the_grid(monkeypatch):
    """259 members on one workgroup of 256 threads: a thread serves two members in turn"""
    monkeypatch.setenv("SOCCER_POP_GRID_BLOCKS", "1")
    b, q = _device_run([60])
    monkeypatch.delenv("SOCCER_POP_GRID_BLOCKS")
    o, ref = _reference_run(5, 4, 0.2, "greedy", "greedy", 259, 5)
    assert_om_population_equal(q.read(), ref.state())
    assert_state_equal(b, o)
    np.testing.assert_array_equal(b.stats()[0], o.hist)
    q.update(*[np.full(259, v, dt) for v, dt in zip((3, 1, 2, 0, 0, 3), DTYPES)])      # update() under the same cap
    r = q.read()
    assert (r["C_a"][:, 3, 2] == ref.C_a[:, 3, 2] + 1).all() and r["steps"] == 61
    b.close()


# ---- 4. per-member hyperparameters ---------------------------------------------------------------------
def test_per_member_hyperparameters():
    n = 67
    rng = np.random.default_rng(3)
    HYPER = dict(alpha=rng.uniform(0.2, 1.0, n), decay=rng.uniform(0.9, 1.0, n), explor=rng.uniform(0.0, 1.0, n))
    gam = rng.uniform(0.0, 0.99, n)
    o = Oracle(5, 4, 0.2, n=n, seed=SEED, autoreset=True)
    ref = OMPopulationNumpy(n, o.nS, gam, **HYPER)
    ref.run(o, o.reset(), T_RUN)
    b = SoccerBatch(n, 5, 4, 0.2, seed=SEED, autoreset=True)
    q = b.om_population(gam, **HYPER)
    b.reset(); q.run(T_RUN)
    got = q.read()
    assert_om_population_equal(got, ref.state())
    assert_state_equal(b, o)
    np.testing.assert_array_equal(q.discount_factor, gam)
    b.close()
    # member i alone: a population created with i's values as scalars has the same member i while i's lane sees the same
    # actions — its own — so with both rows following its own tables it is member i of the run above
    for i in list(range(0, n, 11)) + [n - 1]:
        b1 = SoccerBatch(n, 5, 4, 0.2, seed=SEED, autoreset=True)
        q1 = b1.om_population(float(gam[i]), **{k: float(v[i]) for k, v in HYPER.items()})
        b1.reset(); q1.run(T_RUN)
        one = q1.read(i, 1)
        for k in KEYS:
            assert one[k][0].tobytes() == got[k][i].tobytes(), (i, k)
        b1.close()


# ---- 5. invariance and round trips ------------------------------------------------------------------------
def test_result_does_not_depend_on_the_state_layout(monkeypatch):
    b1, q1 = _device_run([40])
    monkeypatch.setenv("SOCCER_STATE_LAYOUT", "wide")
    b2, q2 = _device_run([40])
    monkeypatch.delenv("SOCCER_STATE_LAYOUT")
    assert b1.state_streams() == 3 and b2.state_streams() == 6
    assert_om_population_equal(q2.read(), q1.read())
    assert_batches_equal(b1, b2)
    b1.close(); b2.close()


def test_read_then_load_of_a_range_on_a_fresh_population_continues_the_same():
    n, first, count = 67, 3, 5
    args = dict(n=n)
    b1, q1 = _device_run([60], **args)
    b2, q2 = _device_run([25], **args)                                  # max_steps = 5: the lanes are in mid-episode
    assert (b2.get_state()["t"] != 0).any()
    ck = q2.read(first, count)
    q3 = b2.om_population(GAMMA, **RUN_KW)                              # a second, fresh population on the same handle
    fresh = q3.read()
    q3.load(ck["Q_a"], ck["Q_b"], ck["C_a"], ck["C_b"], alpha=ck["alpha"], steps=ck["steps"], first=first)
    now = q3.read()
    assert_om_population_equal(q3.read(first, count), ck)
    for k in KEYS:                                                     # nothing outside the range moved
        assert now[k][:first].tobytes() == fresh[k][:first].tobytes() and now[k][first + count:].tobytes() == fresh[k][first + count:].tobytes()
    q3.run(35)                                                         # V and g of the range were derived again on the device
    assert_om_population_equal(q3.read(first, count), q1.read(first, count))
    # one part alone: the rest stays
    q3.load(C_b=ck["C_b"], first=first)
    r = q3.read(first, count)
    assert r["C_b"].tobytes() == ck["C_b"].tobytes() and r["Q_a"].tobytes() == q1.read(first, count)["Q_a"].tobytes()
    # a refused load changes nothing (the Python layer checks first, so straight through the ABI)
    before = q3.read()
    bad = ck["Q_a"].copy(); bad[count - 1, b2.nS - 1, 4, 2] = 1.5
    bad_alpha = ck["alpha"].copy(); bad_alpha[-1] = 2.0
    st = C.c_uint64(99)
    p = {k: ck[k].ctypes.data for k in KEYS}
    for args, msg in (((first, count, bad.ctypes.data, p["Q_b"], p["C_a"], p["C_b"], p["alpha"], C.byref(st)), r"Q_a\[4\]\[%d\]\[4\]\[2\] is outside" % (b2.nS - 1)),
                      ((first, count, p["Q_a"], bad.ctypes.data, None, None, None, None), r"Q_b\[4\]\[%d\]\[4\]\[2\] is outside" % (b2.nS - 1)),
                      ((first, count, p["Q_a"], p["Q_b"], p["C_a"], p["C_b"], bad_alpha.ctypes.data, C.byref(st)), r"alpha\[4\]"),
                      ((65, 5, p["Q_a"], None, None, None, None, C.byref(st)), "outside the population"),
                      ((-1, 1, None, None, None, None, None, C.byref(st)), "outside the population")):
        assert b2.lib.soccer_om_population_load(b2.h, q3.q, *args) == _lib.E_INVALID
        assert re.search(msg, b2.lib.soccer_last_error(b2.h).decode())
        assert_om_population_equal(q3.read(), before)
    with pytest.raises(AssertionError, match="\\[-1, 1\\]"):
        q3.load(bad, ck["Q_b"], first=first)
    row0 = ck["Q_a"].copy(); row0[:, 0] = 7.0                            # row 0 is taken as zeros
    c0 = ck["C_a"].copy(); c0[:, 0] = 9
    q3.load(row0, C_a=c0, first=first)
    r = q3.read(first, count)
    assert (r["Q_a"][:, 0] == 0).all() and (r["C_a"][:, 0] == 0).all()
    b1.close(); b2.close()
    assert q3.q is None and q2.q is None                               # the handle freed both


# ---- 6. frozen lanes, the derived values, the exact scores -------------------------------------------------
def test_lanes_that_were_never_reset_contribute_nothing():
    b, q = _device_run([3], n=67, kw=dict(alpha=0.8, decay=0.5, q_init=0.25), reset=False)
    r = q.read()
    assert b.misuse() == SoccerBatch.MISUSE_FROZEN and r["steps"] == 3
    assert (r["Q_a"][:, 1:] == 0.25).all() and (r["Q_b"][:, 1:] == 0.25).all() and (r["Q_a"][:, 0] == 0).all()
    assert (r["C_a"] == 0).all() and (r["C_b"] == 0).all()
    assert (r["alpha"] == 0.8 * 0.5 * 0.5 * 0.5).all()
    b.close()


def test_derived_values_and_exact_scores_are_each_member_s_own():
    n, m = 67, 5
    b, q = _device_run([200], slip=0.0, n=n, max_steps=100)
    o, ref = _reference_run(5, 4, 0.0, "greedy", "greedy", n, 100, T=200)
    r = q.read()
    assert_om_population_equal(r, ref.state())
    for p, Q, Cn, other in (("a", ref.Q_a, ref.C_a, ref.C_b), ("b", ref.Q_b, ref.C_b, ref.C_a)):
        V, g = derive(Q, Cn)
        assert r["V_" + p].tobytes() == V.tobytes() and r["pi_" + p].tobytes() == np.eye(5)[g].tobytes()
        seen = other.sum(2) > 0
        want = other[seen] / other[seen].sum(1, keepdims=True).astype(np.float64)
        np.testing.assert_allclose(r["model_" + p][seen], want, rtol=0, atol=2e-16)
        assert (r["model_" + p][~seen] == 0.2).all() and seen.any() and not seen.all()
    assert len({r["pi_a"][i].tobytes() for i in range(n)}) > 1         # the members differ
    r5 = q.read(0, m)
    for which, ka, kb in (("greedy", "pi_a", "pi_b"), ("model", "model_a", "model_b")):
        e = q.exploitability(which, theta=1e-6, count=m)
        assert e["gap"].shape == e["v_a"].shape == e["v_b"].shape == (m, b.nS)
        for i in range(m):
            one = pl.exploitability(b, r5[ka][i], r5[kb][i], 1e-6, GAMMA)
            for k in ("v_a", "v_b", "gap"):
                assert e[k][i].tobytes() == one[k].tobytes(), (which, i, k)
        assert (e["gap"][:, 1:] >= -1e-4).all()          # theta / (1 - gamma), with room
        payoff, it = q.cross_play(which, theta=1e-6, count=m)
        want, want_it = b.cross_play(r5[ka], r5[kb], 1e-6, GAMMA)
        assert payoff.tobytes() == want.tobytes() and (it == want_it).all()
        for i in range(m):
            one = b.cross_play(r5[ka][i], r5[kb], 1e-6, GAMMA)[0]
            assert payoff[i].tobytes() == one[0].tobytes(), (which, i)
        g = q.meta_game(which, theta=1e-6, count=m)
        assert g["payoff"].tobytes() == payoff.tobytes() and g["lo"] <= g["value"] <= g["hi"]
    part = q.exploitability("model", theta=1e-6, first=2, count=2)
    assert part["gap"].tobytes() == q.exploitability("model", theta=1e-6, count=m)["gap"][2:4].tobytes()
    with pytest.raises(AssertionError, match="'greedy' or 'model'"):
        q.exploitability("avg")
    b.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=False)
    with pytest.raises(AssertionError, match="soccer_om_population_create needs a handle created with SOCCER_F_AUTORESET"):
        b.om_population(GAMMA)
    b.close()
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=True)
    b.set_policy("player_b", np.zeros(b.nS, np.int8))
    with pytest.raises(AssertionError, match="soccer_om_population_create needs a two-player handle"):
        b.om_population(GAMMA)
    b.set_policy("player_b", None)
    q = b.om_population(GAMMA)
    with pytest.raises(AssertionError, match="outside the population"):
        q.read(60, 5)
    st = C.c_uint64()
    for first, count in ((65, 0), (0, 65), (-1, 2), (3, -1), (2 ** 62, 2 ** 62)):
        assert b.lib.soccer_om_population_read(b.h, q.q, first, count, None, None, None, None, None, C.byref(st)) == _lib.E_INVALID
        assert "soccer_om_population_read: members" in b.lib.soccer_last_error(b.h).decode()
    dev = [b.alloc(64, dt).fill(0) for dt in DTYPES]
    b.sync()
    b.graph_begin()
    b.rollout(2, sample_actions=True)           # (something to capture; never replayed)
    for call, name in ((lambda: q.run(1), "soccer_om_population_run"), (lambda: q.read(), "soccer_om_population_read"),
                       (lambda: q.load(np.zeros((64, b.nS, 5, 5))), "soccer_om_population_load"),
                       (lambda: b.om_population(GAMMA), "soccer_om_population_create"),
                       (lambda: q.update(*dev), "soccer_om_population_update"), (lambda: q.steps, "soccer_om_population_read")):
        with pytest.raises(RuntimeError, match=name + " during graph capture"):
            call()
    b.graph_destroy(b.graph_end())
    other = SoccerBatch(8, 5, 4, 0.0, autoreset=True)
    with pytest.raises(AssertionError, match="soccer_om_population_run: not a population of this handle"):
        other._check(other.lib.soccer_om_population_run(other.h, q.q, 1))
    other.close()
    qq = b.q_population(GAMMA)                  # a population of another kind is not one of these
    with pytest.raises(AssertionError, match="not a population of this handle"):
        b._check(b.lib.soccer_om_population_run(b.h, qq.q, 1))
    with pytest.raises(AssertionError, match="soccer_om_population_run: n_steps must be >= 0"):
        q.run(-1)
    assert b.lib.soccer_om_population_update(b.h, q.q, dev[0].ptr, None, None, None, None, None) == _lib.E_INVALID
    assert "soccer_om_population_update: all six" in b.lib.soccer_last_error(b.h).decode()
    # the library's own range checks (the Python layer checks first, so straight through the ABI)
    uniform = np.full((b.nS, 5), 0.2)
    bad_row = uniform.copy(); bad_row[3] = [0.5, 0.5, 0.5, 0.0, 0.0]
    ok64 = np.full(64, 0.5)

    def arr(i, v):
        a = ok64.copy(); a[i] = v
        return a
    keep = [arr(7, 1.0), arr(8, -0.5), arr(9, 0.0), arr(63, 2.0)]
    for fields, msg in ((dict(discount_factor=1.0), "discount_factor"), (dict(alpha=-0.5), "alpha"), (dict(decay=0.0), "decay"),
                        (dict(explor=2.0), "explor"), (dict(q_init=-1.5), "q_init"), (dict(act_a=7), "act_a"), (dict(act_b=-1), "act_b"),
                        (dict(act_a=_lib.QL_FIXED), "policy_a"), (dict(policy_b=uniform.ctypes.data), "policy_b"),
                        (dict(act_a=_lib.QL_FIXED, policy_a=bad_row.ctypes.data), "policy_a\\[3\\] does not sum to 1"),
                        (dict(discount_factor_per_member=keep[0].ctypes.data), "discount_factor_per_member\\[7\\]"),
                        (dict(alpha_per_member=keep[1].ctypes.data), "alpha_per_member\\[8\\]"),
                        (dict(decay_per_member=keep[2].ctypes.data), "decay_per_member\\[9\\]"),
                        (dict(explor_per_member=keep[3].ctypes.data), "explor_per_member\\[63\\]")):
        cfg = _lib.OMPopulationConfig(0.9, 1.0, 0.5, 0.2, 1.0, 0, 0, None, None, None, None, None, None)
        for k, v in fields.items():
            setattr(cfg, k, v)
        out = C.c_void_p()
        assert b.lib.soccer_om_population_create(b.h, C.byref(cfg), C.byref(out)) == _lib.E_INVALID and not out.value
        assert re.search(msg, b.lib.soccer_last_error(b.h).decode()), (msg, b.lib.soccer_last_error(b.h))
    ql = b.q_learning(GAMMA)                    # the other learners share the handle
    b.reset(); q.run(2); ql.run(2); qq.run(2)
    assert q.steps == 2 and ql.steps == 2 and b.tick == 7 and b.misuse() == 0
    b.close()                                   # with live learners: the handle frees them
    assert qq.q is None and q.q is None
    q.close()                                   # the wrapper knows
    with pytest.raises(AssertionError, match="handle is NULL"):        # use after the handle's close
        q.run(1)
    with pytest.raises(AssertionError, match="handle is NULL"):
        q.read(0, 1)


# ---- 8. it learns -----------------------------------------------------------------------------------------
def test_every_member_learns_the_best_response_values():
    """The learning run of tests/test_om_population_np.py on the device, same n, T and seed, so the restatement's figure is the
    device's (test 2 pins the bits): (greedy, uniform), 64 one-actor learners from Q = 0, alpha 1 -> 0.01; the population mean
    of the mean over the live states of |V_a - V(A's exact best response to a uniform B)| stays under BOUND.  Printed beside
    what q_population reaches in the same run."""
    c = LEARN
    env = VectorSoccerEnv(c["n"], c["width"], c["height"], c["slip"], seed=c["seed"], autoreset=True)
    want = pl.best_response(env, np.full((env.nS, 5), 0.2), 1, 1e-10, c["gamma"])[1]
    kw = dict(alpha=c["alpha"], decay=0.01 ** (1.0 / c["T"]), explor=c["explor"], q_init=c["q_init"], act_a="greedy", act_b="uniform")
    q = env.om_population(c["gamma"], **kw)
    env.reset()
    env._batch.sync()
    t0 = time.perf_counter()
    q.run(c["T"])
    steps = q.steps                             # synchronises
    wall = time.perf_counter() - t0
    r = q.read()
    err = np.abs(r["V_a"] - want)[:, 1:].mean(1)
    q.close()
    env2 = VectorSoccerEnv(c["n"], c["width"], c["height"], c["slip"], seed=c["seed"], autoreset=True)
    qq = env2.q_population(c["gamma"], **kw)
    env2.reset(); qq.run(c["T"])
    err_q = np.abs(qq.read()["V_a"] - want)[:, 1:].mean(1)
    print("(greedy, uniform), %d members x %d steps: population mean %.6f (members %.6f .. %.6f); run() took %.3f s = %.2f us per "
          "step; q_population in the same run: %.6f" % (c["n"], c["T"], err.mean(), err.min(), err.max(), wall, wall / c["T"] * 1e6, err_q.mean()))
    assert steps == c["T"] and np.abs(r["alpha"] - 0.01).max() < 1e-9
    assert err.mean() <= BOUND
    pa, pb, Va, Vb, Qa, Qb, al = pl.om_population(env, 50, c["gamma"], q_init=0.0, act_b="uniform", first=3, count=5)      # the planner-style entry point
    assert pa.shape == pb.shape == (5, env.nS, 5) and Qa.shape == Qb.shape == (5, env.nS, 5, 5)
    assert Va.shape == Vb.shape == (5, env.nS) and al.shape == (5,) and (pa.sum(2) == 1).all()
    env.close(); env2.close()
