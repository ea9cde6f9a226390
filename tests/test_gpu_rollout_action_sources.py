"""batched_rollout / batched_rollout_ex with actions keyed by the lane's current observation — mixed-policy rows, fixed int8
policies, against streamed or sampled opponents — on every table placement the launch can take (LDS under 48 KB, LDS above
48 KB behind the raised limit, global memory) and on the per-lane kernel, every lane of every step against the CPU oracle.
Each case also asks the handle which shape it launched (SoccerBatch.rollout_shape) and checks that against its arguments; the
last test of the module asserts which placements the cases reached.

The tables are full of what a solved game's strategies are full of: one-hot rows and rows with zero-probability actions, i.e.
equal neighbouring thresholds and thresholds at 0 and at 32768 (above 32768 is out of contract and not tested).  Row 0 — what a
lane parked in a goal tuple looks up — is a one-hot on a non-zero action and policy[0] is non-zero."""
import os
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch, VectorSoccerEnv
from gym_soccer_littman94_amd import planners as pl
from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rollout_shape_cases import (BYTE_PARALLEL, GLOBAL, LDS, NONE, PER_LANE, SLIP_ROWS_BYTES, SOURCES,  # noqa: E402,F401
                                 STAGING_BYTES, _check_shape, _table_bytes)
from test_gpu_swar import _oracle_rollout, _rollout_vs_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

N, T = 4096 + 3, 48             # a ragged tail: the last three lanes go through the per-lane kernel on the same ticks
STRIDE = 4096 + 4               # (rows a multiple of 4 apart, or the whole call would)
OFFSET = 4 * 1000003
# (width, height, slip, source, kernel, slip selection).  nS: 5x4 761, 7x6 3445, 9x6 5725, 10x7 9661, 11x7 11705.
CASES = [
    # 5x4: every table in LDS under 48 KB; slip 0 / by table (0.2) / one by one (0.03)
    (5, 4, 0.0, "both_mixed", BYTE_PARALLEL, 0), (5, 4, 0.2, "mix_a", BYTE_PARALLEL, 2), (5, 4, 0.03, "mix_b", BYTE_PARALLEL, 1),
    (5, 4, 0.0, "fixed_a_stream_b", BYTE_PARALLEL, 0), (5, 4, 0.0, "fixed_b_stream_a", BYTE_PARALLEL, 0),
    (5, 4, 0.2, "fixed_a_uniform_b", BYTE_PARALLEL, 2), (5, 4, 0.0, "fixed_b_mix_a", BYTE_PARALLEL, 0),
    # 7x6: 55 KB of 16-byte rows, 62 KB of 8 + 1 byte tables: LDS behind the raised limit, below 64 KB
    (7, 6, 0.2, "both_mixed", BYTE_PARALLEL, 2), (7, 6, 0.2, "mix_a", BYTE_PARALLEL, 2), (7, 6, 0.2, "mix_b", BYTE_PARALLEL, 2),
    (7, 6, 0.2, "fixed_a_stream_b", BYTE_PARALLEL, 2), (7, 6, 0.2, "fixed_b_stream_a", BYTE_PARALLEL, 2),
    (7, 6, 0.2, "fixed_a_uniform_b", BYTE_PARALLEL, 2), (7, 6, 0.2, "fixed_b_mix_a", BYTE_PARALLEL, 2), (7, 6, 0.2, "uniform", BYTE_PARALLEL, 2),
    # 9x6: 92 KB / 103 KB: LDS where a workgroup may have 160 KB
    (9, 6, 0.0, "both_mixed", BYTE_PARALLEL, 0), (9, 6, 0.03, "both_mixed", BYTE_PARALLEL, 1),
    (9, 6, 0.03, "fixed_b_stream_a", BYTE_PARALLEL, 1), (9, 6, 0.03, "fixed_a_stream_b", BYTE_PARALLEL, 1),
    # 10x7: the 16-byte rows fit at slip 0 and not next to the static slip table of slip 0.2; the 8 + 1 byte form never fits
    (10, 7, 0.0, "both_mixed", BYTE_PARALLEL, 0), (10, 7, 0.2, "both_mixed", BYTE_PARALLEL, 2),
    (10, 7, 0.0, "fixed_a_stream_b", BYTE_PARALLEL, 0), (10, 7, 0.2, "fixed_b_stream_a", BYTE_PARALLEL, 2), (10, 7, 0.0, "mix_a", BYTE_PARALLEL, 0),
    # 11x7: everything in global memory
    (11, 7, 0.2, "both_mixed", BYTE_PARALLEL, 2), (11, 7, 0.2, "mix_b", BYTE_PARALLEL, 2),
    (11, 7, 0.2, "fixed_a_uniform_b", BYTE_PARALLEL, 2), (11, 7, 0.2, "fixed_b_mix_a", BYTE_PARALLEL, 2),
    # rollout_kernel<.., DYN = true>: beyond the byte arithmetic (13x9), and 5x4 at slip 0.33 with SOCCER_ROLLOUT=1.  (0.33 has an
    # exact integer decision, so left alone it takes the byte-parallel kernel with the table selection: the last case.  The
    # per-lane kernel is what a slip without one gets, and SOCCER_ROLLOUT=1 is how a test reaches it on a pitch this small.)
    (13, 9, 0.2, "both_mixed", PER_LANE, 1), (13, 9, 0.2, "fixed_a_stream_b", PER_LANE, 1), (13, 9, 0.2, "fixed_b_mix_a", PER_LANE, 1),
    (5, 4, 0.33, "mix_a", PER_LANE, 1), (5, 4, 0.33, "fixed_b_stream_a", PER_LANE, 1), (5, 4, 0.33, "fixed_a_uniform_b", PER_LANE, 1),
    (5, 4, 0.33, "both_mixed", BYTE_PARALLEL, 2),
    (9, 6, 0.0, "fixed_a_uniform_b", BYTE_PARALLEL, 0),         # 103 KB of 8 + 1 byte tables, no staging area
]
TABLE_SEEDS = {19: 2000}        # 10x7 at slip 0 starts every lane in one of two tuples: a draw of tables under which both sides score
_REACHED = {}       # case -> the shape it reported (test_zz_the_cases_reached_every_placement)


def _threshold_rows(rng, nS):
    """uint16[nS, 4] cumulative thresholds of integer weights that sum to 32768: a third of the rows one-hot, a third with
    one to four actions of weight zero, the rest Dirichlet(0.6); row 0 one-hot on a non-zero action"""
    p = rng.dirichlet(np.ones(5) * 0.6, size=nS)
    kind = rng.integers(0, 3, size=nS)
    for s in np.flatnonzero(kind == 1):
        p[s, rng.choice(5, size=rng.integers(1, 5), replace=False)] = 0.0
    w = np.floor(p / p.sum(1, keepdims=True) * 32768.0).astype(np.int64)
    w[np.arange(nS), p.argmax(1)] += 32768 - w.sum(1)                       # the remainder goes to the row's largest weight
    hot = np.flatnonzero(kind == 0)
    w[hot] = 32768 * np.eye(5, dtype=np.int64)[rng.integers(0, 5, size=hot.size)]
    w[0] = 32768 * np.eye(5, dtype=np.int64)[rng.integers(1, 5)]
    assert (w >= 0).all() and (w.sum(1) == 32768).all()
    return np.ascontiguousarray(np.cumsum(w, axis=1)[:, :4].astype(np.uint16))


def _fixed_policy(rng, nS):
    policy = rng.integers(0, 5, size=nS).astype(np.int8)
    policy[0] = rng.integers(1, 5)
    return policy


def _inputs(rng, nS, source, n, steps):
    sample, use_a, use_b, fixed = SOURCES[source]
    mix = (_threshold_rows(rng, nS) if use_a else None, _threshold_rows(rng, nS) if use_b else None) if (use_a or use_b) else None
    policy = _fixed_policy(rng, nS) if fixed else None
    acts = None if sample else rng.integers(0, 5, size=(steps, 2, n), dtype=np.int8)
    return dict(sample=sample, mix=mix, policy=policy, fixed=fixed, acts=acts)


def _floors(source):
    """the conditions a default-shape case puts on its inputs, checked on the oracle's run before the device is looked at"""
    sample, use_a, use_b, fixed = SOURCES[source]
    def check(seen):
        for side, counts in seen["draws"].items():
            assert counts.min() >= 1000, "%s drew %s" % (side, counts)
        assert seen["plus"] >= 200 and seen["minus"] >= 200, "episodes ending +1 / -1: %d / %d" % (seen["plus"], seen["minus"])
        if use_a or use_b:
            assert seen["degenerate_rows"] >= 250, "visited rows with a threshold at 0 or 32768: %d" % seen["degenerate_rows"]
    return check


def _tuples(o, fl):
    """flat table indices -> (row_a, col_a, row_b, col_b, poss)"""
    W, H = o.W, o.H
    p_ = fl & 1; r = fl >> 1; yb = r % W; r //= W; xb = r % H; r //= H; ya = r % W; xa = r // W
    return xa, ya, xb, yb, p_


def _start_on_the_boundary_rows(b, o):
    """after the reset, lanes 1 and 6 are moved to the tuple numbered nS - 1 and lane 2 to the one numbered 1, inside groups whose
    other lanes stay where the reset put them: the last and the first live row of every table are looked up at step 0"""
    lut, kind, *_ = o.tables()
    st = b.get_state()
    for lane, s in ((1, o.nS - 1), (2, 1), (6, o.nS - 1)):
        xa, ya, xb, yb, p_ = _tuples(o, np.flatnonzero((lut == s) & (kind == 1))[:1])
        for name, v in (("row_a", xa), ("col_a", ya), ("row_b", xb), ("col_b", yb), ("poss", p_)):
            st[name][lane] = v[0]
    for x in (b, o):
        x.set_state(st["row_a"], st["col_a"], st["row_b"], st["col_b"], st["poss"], t=st["t"], needs_reset=st["needs_reset"])


def _case_id(c):
    return "%dx%d-slip%s-%s" % (c[0], c[1], c[2], c[3])


@pytest.mark.parametrize("index", range(len(CASES)), ids=[_case_id(c) for c in CASES])
def test_observation_keyed_rollout_every_lane_every_step(index, monkeypatch):
    w, h, slip, source, kernel, slip_sel = CASES[index]
    if kernel == PER_LANE and w * h <= 100:
        monkeypatch.setenv("SOCCER_ROLLOUT", "1")           # read by soccer_create
    rng = np.random.default_rng(TABLE_SEEDS.get(index, 1000 + index))
    offset = OFFSET if index & 1 else 0
    extras = bool((index >> 1) & 1)
    o = Oracle(w, h, slip, n=N, seed=40 + index, autoreset=True, lane_offset=offset)
    inp = _inputs(rng, o.nS, source, N, T)
    b = SoccerBatch(N, w, h, slip, seed=40 + index, autoreset=True, lane_offset=offset)
    if inp["fixed"]:
        b.set_policy(inp["fixed"], inp["policy"])
    b.reset(); o.reset()
    _start_on_the_boundary_rows(b, o)
    _rollout_vs_oracle(b, o, inp["acts"], T, N, sample=inp["sample"], mix=inp["mix"], policy=inp["policy"], fixed=inp["fixed"],
                       extras=extras, precheck=_floors(source), strict=True, stride=STRIDE)
    sh = b.rollout_shape()
    print("%-32s %s" % (_case_id(CASES[index]), sh))
    _check_shape(sh, o.nS, N, T, source, kernel, slip_sel, extras)
    _REACHED[index] = sh
    b.close()


def test_rollout_shape_before_the_first_rollout_and_after_plain_streams():
    n = 4096
    b = SoccerBatch(n, 5, 4, 0.0, seed=1, autoreset=True)
    sh = b.rollout_shape()
    assert sh["kernel"] == 0 and sh["lds_limit"] >= 64 * 1024 and sh["parts"] == 0 and sh["dynamic_lds_bytes"] == 0
    b.reset()
    b.step(b.alloc(n, np.int8).fill(0), b.alloc(n, np.int8).fill(0))
    assert b.rollout_shape()["kernel"] == 0                 # a step is not a rollout
    A = b.alloc((3, n), np.int8).fill(1)
    b.rollout(3, A, A, act_stride=n)
    sh = b.rollout_shape()
    assert (sh["kernel"], sh["action_source"], sh["table_placement"], sh["tail"], sh["parts"], sh["chunks"]) == (BYTE_PARALLEL, 0, NONE, 0, 1, 1)
    assert sh["dynamic_lds_bytes"] == SLIP_ROWS_BYTES + STAGING_BYTES
    b.close()


def _special_state(rng, o, n):
    """a third of the lanes in goal tuples (needs_reset 0: the absorbing step), a third frozen, the rest live"""
    lut, kind, *_ = o.tables()
    live, goal = np.flatnonzero(kind == 1), np.flatnonzero(kind == 2)
    fl = np.where(rng.random(n) < 0.33, rng.choice(goal, n), rng.choice(live, n))
    nr = (rng.random(n) < 0.33).astype(np.uint8)
    t0 = rng.choice([0, 3, 97, 99, 100], n).astype(np.uint8)
    return _tuples(o, fl), t0, nr


@pytest.mark.parametrize("w,h,slip", [(7, 6, 0.2), (5, 4, 0.0)])
@pytest.mark.parametrize("autoreset", [True, False])
@pytest.mark.parametrize("source", ["both_mixed", "fixed_a_stream_b"])
def test_observation_keyed_rollout_special_lanes(w, h, slip, autoreset, source):
    """frozen lanes and lanes parked in goal tuples (which look up row 0) inside one thread's group of four, with and
    without auto-reset; then a second rollout from the state the first one left"""
    rng = np.random.default_rng(77 + w + 2 * autoreset)
    o = Oracle(w, h, slip, n=N, seed=31, autoreset=autoreset)
    b = SoccerBatch(N, w, h, slip, seed=31, autoreset=autoreset)
    inp = _inputs(rng, o.nS, source, N, 2 * T)
    if inp["fixed"]:
        b.set_policy(inp["fixed"], inp["policy"])
    tup, t0, nr = _special_state(rng, o, N)
    for x in (b, o):
        x.set_state(*tup, t=t0, needs_reset=nr)
    assert nr.any() and not nr.all()
    for part in range(2):
        acts = None if inp["acts"] is None else inp["acts"][part * T:(part + 1) * T]
        _rollout_vs_oracle(b, o, acts, T, N, sample=inp["sample"], mix=inp["mix"], policy=inp["policy"], fixed=inp["fixed"],
                           extras=bool(part), strict=True, stride=STRIDE)
        assert b.misuse() == SoccerBatch.MISUSE_FROZEN          # frozen lanes were stepped: the sticky flag
        _check_shape(b.rollout_shape(), o.nS, N, T, source, BYTE_PARALLEL, 2 if slip else 0, bool(part))
    b.close()


@pytest.mark.parametrize("w,h,slip,source", [(7, 6, 0.2, "both_mixed"), (9, 6, 0.0, "fixed_b_stream_a")])
def test_observation_keyed_rollout_on_the_wide_state_layout(w, h, slip, source, monkeypatch):
    monkeypatch.setenv("SOCCER_STATE_LAYOUT", "wide")
    b = SoccerBatch(N, w, h, slip, seed=12, autoreset=True, lane_offset=OFFSET)
    monkeypatch.delenv("SOCCER_STATE_LAYOUT")
    assert b.state_streams() == 6
    rng = np.random.default_rng(5 + w)
    o = Oracle(w, h, slip, n=N, seed=12, autoreset=True, lane_offset=OFFSET)
    inp = _inputs(rng, o.nS, source, N, T)
    if inp["fixed"]:
        b.set_policy(inp["fixed"], inp["policy"])
    b.reset(); o.reset()
    _rollout_vs_oracle(b, o, inp["acts"], T, N, sample=inp["sample"], mix=inp["mix"], policy=inp["policy"], fixed=inp["fixed"],
                       extras=True, precheck=_floors(source), strict=True, stride=STRIDE)
    _check_shape(b.rollout_shape(), o.nS, N, T, source, BYTE_PARALLEL, 2 if slip else 0, True)
    b.close()


def test_observation_keyed_rollout_split_into_several_launches(monkeypatch):
    """SOCCER_SWAR_LAUNCH_LANES = 4096: three parts, a short one and a ragged tail; every part stages its own tables"""
    monkeypatch.setenv("SOCCER_SWAR_LAUNCH_LANES", "4096")
    n = 3 * 4096 + 1028 + 3
    b = SoccerBatch(n, 7, 6, 0.2, seed=29, autoreset=True, lane_offset=4 * 55)
    monkeypatch.delenv("SOCCER_SWAR_LAUNCH_LANES")
    o = Oracle(7, 6, 0.2, n=n, seed=29, autoreset=True, lane_offset=4 * 55)
    inp = _inputs(np.random.default_rng(13), o.nS, "both_mixed", n, T)
    b.reset(); o.reset()
    _rollout_vs_oracle(b, o, None, T, n, sample=True, mix=inp["mix"], extras=False, precheck=_floors("both_mixed"), strict=True,
                       stride=n + 1)
    sh = b.rollout_shape()
    assert sh["parts"] == 4
    _check_shape(sh, o.nS, n, T, "both_mixed", BYTE_PARALLEL, 2, False, launch_lanes=4096)
    b.close()


@pytest.mark.parametrize("slip,max_steps,source", [(0.2, 1, "both_mixed"), (0.0, 100, "fixed_a_stream_b")])
def test_observation_keyed_rollout_longer_than_one_chunk(slip, max_steps, source):
    """4096 + 9 steps: two launches on consecutive ticks, the second one's streams offset by the OUTPUT stride.  With
    max_steps = 1 every lane finishes an episode at every step, so the 16-bit per-chunk episode counters end the first chunk
    at 4096."""
    n, steps = 1024, 4096 + 9
    rng = np.random.default_rng(3 + max_steps)
    o = Oracle(5, 4, slip, n=n, seed=19, autoreset=True, max_steps=max_steps)
    b = SoccerBatch(n, 5, 4, slip, seed=19, autoreset=True, max_steps=max_steps)
    inp = _inputs(rng, o.nS, source, n, steps)
    if inp["fixed"]:
        b.set_policy(inp["fixed"], inp["policy"])
    b.reset(); o.reset()

    def check(seen):
        if max_steps == 1:
            assert (seen["episodes"] == steps).all()
        else:
            assert seen["plus"] >= 200 and seen["minus"] >= 200
    ec, eps = _rollout_vs_oracle(b, o, inp["acts"], steps, n, sample=inp["sample"], mix=inp["mix"], policy=inp["policy"],
                                 fixed=inp["fixed"], extras=True, precheck=check, strict=True)
    np.testing.assert_array_equal(ec, eps)
    sh = b.rollout_shape()
    assert sh["chunks"] == 2
    _check_shape(sh, o.nS, n, steps, source, BYTE_PARALLEL, 2 if slip else 0, True)
    b.close()


def _check_venv_rollout(venv, o, steps, probs=None, policy=None, fixed=None, acts=None):
    """VectorSoccerEnv.rollout against the oracle's replay, every step (as test_gpu_minimax.py's config-5 test does)"""
    obs0, _ = venv.reset()
    ag = venv.return_agent[0]
    cur = o.reset()
    np.testing.assert_array_equal(obs0[ag], cur)
    mix = None if probs is None else tuple(SoccerBatch.mixed_policy_thresholds(p) for p in probs)
    want, seen = _oracle_rollout(o, acts, steps, o.n, sample=acts is None, mix=mix, policy=policy, fixed=fixed)
    if acts is None:
        O, R, TE, TR, _ = venv.rollout(steps, sample_actions=True, mixed_policies={"player_a": probs[0], "player_b": probs[1]})
    else:
        O, R, TE, TR, _ = venv.rollout(steps, actions={ag: acts[:, 0 if ag == "player_a" else 1]})
    sign = 1.0 if ag == "player_a" else -1.0
    for t, c in enumerate(want):
        np.testing.assert_array_equal(O[ag][t], c["obs"], err_msg="obs %d" % t)
        np.testing.assert_array_equal(R[ag][t], sign * c["reward"].astype(np.float32), err_msg="reward %d" % t)
        np.testing.assert_array_equal(TE[ag][t], c["terminated"].astype(bool))
        np.testing.assert_array_equal(TR[ag][t], c["truncated"].astype(bool))
    np.testing.assert_array_equal(venv.episode_histogram(), o.hist)
    return seen


def test_minimax_strategies_of_7x6_rolled_out_through_the_vector_env():
    """planners.minimax_value_iteration on 7x6, slip 0.2 (3445 states: both tables behind the raised LDS limit) -> both
    strategies into VectorSoccerEnv.rollout(sample_actions=True, mixed_policies=...), 4096 lanes x 60 steps"""
    n, steps = 4096, 60
    solver = SoccerBatch(1, 7, 6, 0.2)
    pa, pb, V, Q, k = pl.minimax_value_iteration(solver, 1e-10, 0.9)
    solver.close()
    ta, tb = SoccerBatch.mixed_policy_thresholds(pa), SoccerBatch.mixed_policy_thresholds(pb)
    pure = int(((ta == 0) | (ta == 32768)).any(1).sum()), int(((tb == 0) | (tb == 32768)).any(1).sum())
    print("7x6 slip 0.2 minimax strategies after %d sweeps: rows with a threshold at 0 or 32768: A %d, B %d of %d" % ((k,) + pure + (len(ta),)))
    venv = VectorSoccerEnv(n, 7, 6, 0.2, seed=1994)
    o = Oracle(7, 6, 0.2, n=n, seed=1994, autoreset=True)
    seen = _check_venv_rollout(venv, o, steps, probs=(pa, pb))
    assert seen["degenerate_rows"] >= 250       # the strategies of a solved game: rows with zero-probability actions are what lanes visit
    sh = venv._batch.rollout_shape()
    _check_shape(sh, o.nS, n, steps, "both_mixed", BYTE_PARALLEL, 2, False)
    assert sh["dynamic_lds_bytes"] > 48 * 1024 or sh["lds_limit"] < 64 * 1024
    venv.close()


def test_single_agent_vector_env_of_9x6_rolled_out():
    """VectorSoccerEnv(player_b_policy=...) on 9x6: rollout() with the learner's action stream (T - 1 fused steps, the fixed
    side's 5725-entry policy next to 92 KB of unused row space, and one full step)"""
    n, steps = 4096, 60
    rng = np.random.default_rng(9)
    o = Oracle(9, 6, 0.0, n=n, seed=7, autoreset=True)
    policy = _fixed_policy(rng, o.nS)
    acts = rng.integers(0, 5, size=(steps, 2, n), dtype=np.int8)
    venv = VectorSoccerEnv(n, 9, 6, 0.0, seed=7, player_b_policy=policy)
    _check_venv_rollout(venv, o, steps, policy=policy, fixed="player_b", acts=acts)
    _check_shape(venv._batch.rollout_shape(), o.nS, n, steps - 1, "fixed_b_stream_a", BYTE_PARALLEL, 0, False)
    venv.close()


def test_zz_the_cases_reached_every_placement():
    """which placement every parametrised case above took on this device, and — where a workgroup may have 160 KB — that
    every byte-parallel action-source shape that looks tables up met every placement it can reach"""
    assert sorted(_REACHED) == list(range(len(CASES))), "run the whole module: this test reads what the cases above reported"
    limit = _REACHED[0]["lds_limit"]
    where = {}
    for i, sh in sorted(_REACHED.items()):
        place = "per-lane kernel" if sh["kernel"] == PER_LANE else ("none", "LDS", "global")[sh["table_placement"]]
        if sh["kernel"] == BYTE_PARALLEL and sh["table_placement"] == LDS:
            place += " > 48 KB" if sh["dynamic_lds_bytes"] > 48 * 1024 else " < 48 KB"
            where.setdefault(sh["action_source"], set()).add(place)
        elif sh["kernel"] == BYTE_PARALLEL and sh["table_placement"] == GLOBAL:
            where.setdefault(sh["action_source"], set()).add(place)
        print("%-32s action source %d  slip selection %d  %-16s dynamic LDS %6d B" %
              (_case_id(CASES[i]), sh["action_source"], sh["slip_selection"], place, sh["dynamic_lds_bytes"]))
    if limit < 160 * 1024:
        pytest.skip("a workgroup of this device may have %d B of LDS: the placements above are what it reaches" % limit)
    both = {"LDS < 48 KB", "LDS > 48 KB"}
    assert where[2] == both                     # never global by construction
    for dm in (3, 4, 5):
        assert where[dm] == both | {"global"}, (dm, where[dm])
    at = {(c[2], c[3]): _REACHED[i] for i, c in enumerate(CASES) if c[:2] == (10, 7)}
    assert at[(0.0, "both_mixed")]["table_placement"] == LDS and at[(0.2, "both_mixed")]["table_placement"] == GLOBAL
    # every slip selection met each of the four shapes
    for dm in (2, 3, 4, 5):
        assert {sh["slip_selection"] for sh in _REACHED.values() if sh["kernel"] == BYTE_PARALLEL and sh["action_source"] == dm} == {0, 1, 2}, dm
