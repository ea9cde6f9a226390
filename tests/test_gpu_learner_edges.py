"""-m gpu: the three on-device learners (minimax-Q, the independent Q-learners, WoLF-PHC) against their numpy restatements, bit
for bit, away from the corner their own suites test in: episodes that truncate (T, C), frozen, goal-parked and nearly-out-of-time
lanes in one launch (S), grid-stride loops that wrap in run() and update() (W, U), the integer sums at their stated worst case
(U), act kernels with more than 48 KB of dynamic LDS (L), act kernels whose observation table stays in global memory (G) and a lane offset that carries lane ids across 2^32 (O).  The cases are
defined in tests/test_learner_edges_np.py, which also shows without a GPU that each reaches its path.  No tolerances."""
import os
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch, _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_q_learning import _random_batch, assert_batches_equal, assert_state_equal  # noqa: E402
from test_learner_edges_np import (CASES, GAMMA, KW, LEARNERS, MAX_LANES, SEED, assert_read_equal, grid_wrap_case, new_restatement,  # noqa: E402
                                   reference)
from test_matrix_game_host import build_games_host  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_games_host(tmp_path_factory.mktemp("games_edges_gpu"))


def new_batch(c):
    return SoccerBatch(c["n"], c["w"], c["h"], c["slip"], seed=SEED, autoreset=True, max_steps=c["max_steps"],
                       lane_offset=c.get("lane_offset", 0))


def new_learner(b, learner, **over):
    kw = dict(KW[learner]); kw.update(over)
    return getattr(b, learner)(GAMMA, **kw)


def device_run(learner, c, parts, st=None):
    """a fresh handle and learner: reset, the case's special lanes, then run() part by part"""
    b = new_batch(c)
    q = new_learner(b, learner)
    b.reset()
    if st is not None:
        b.set_state(**st)
    for t in parts:
        q.run(t)
    return b, q


def assert_equals_reference(learner, b, q, o, ref, misuse=0):
    """the full read(), the state streams, the tick, the episode histogram and the misuse word"""
    assert_read_equal(learner, q.read(), ref.state())
    assert_state_equal(b, o)
    assert b.tick == o.tick
    hist, mis = b.stats()
    np.testing.assert_array_equal(hist, o.hist)
    assert mis == misuse and (o.misuse > 0) == (misuse == SoccerBatch.MISUSE_FROZEN)
    assert hist.sum() > 0 and q.steps == ref.steps


def load_checkpoint(learner, q, ck):
    if learner == "minimax_q":
        q.load(ck["Q"], visits=ck["visits"], alpha=ck["alpha"], steps=ck["steps"])
    elif learner == "q_learning":
        q.load(ck["Q_a"], ck["Q_b"], visits=ck["visits"], alpha=ck["alpha"], steps=ck["steps"])
    else:
        q.load(ck["Q_a"], ck["Q_b"], pi_a=ck["pi_a"], pi_b=ck["pi_b"], avg_a=ck["avg_a"], avg_b=ck["avg_b"], visits=ck["visits"],
               updates=ck["updates"], alpha=ck["alpha"], dscale=ck["dscale"], steps=ck["steps"])


# ---- T: truncation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["T", "T every transition truncates"])
@pytest.mark.parametrize("learner", LEARNERS)
def test_truncated_episodes_bootstrap_from_final_obs(host, learner, name):
    c = CASES[name]
    o, ref = reference(learner, name, host)[:2]
    assert ref.n_truncated > ref.n_terminated                  # truncated transitions that are not terminated
    assert name == "T" or (ref.n_truncated, ref.n_terminated) == (c["n"] * c["T"], 0)
    b, q = device_run(learner, c, [c["T"]])
    assert_equals_reference(learner, b, q, o, ref)
    b.close()


# ---- C: composition across truncations --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("learner", LEARNERS)
def test_runs_compose_across_truncations(host, learner):
    c = CASES["T"]
    o, ref = reference(learner, "T", host)[:2]
    assert ref.n_truncated > ref.n_terminated > 0
    b1, q1 = device_run(learner, c, [13, 27])
    assert_equals_reference(learner, b1, q1, o, ref)
    b2, q2 = device_run(learner, c, [13])
    ck = q2.read()
    q3 = new_learner(b2, learner)                              # a fresh learner on the same handle takes over
    load_checkpoint(learner, q3, ck)
    assert_read_equal(learner, q3.read(), ck)
    q3.run(27)
    assert_equals_reference(learner, b2, q3, o, ref)
    assert_batches_equal(b1, b2)
    b1.close(); b2.close()


# ---- S: special lanes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S", "S uint8 end of t"])
@pytest.mark.parametrize("learner", LEARNERS)
def test_frozen_parked_and_late_lanes_beside_plain_ones(host, learner, name):
    c = CASES[name]
    o, ref, st, m = reference(learner, name, host)
    assert ref.n_left_out == 820 * c["T"] + 469 and ref.n_truncated >= 256 and int(st["t"].max()) == c["max_steps"] - 1
    b = new_batch(c)
    q = new_learner(b, learner)
    b.reset()
    b.set_state(**st)
    before = b.get_state()
    q.run(c["T"])
    assert_equals_reference(learner, b, q, o, ref, misuse=SoccerBatch.MISUSE_FROZEN)
    after = b.get_state()
    for k in before:
        assert after[k][m["frozen"]].tobytes() == before[k][m["frozen"]].tobytes(), k
    assert int(q.read()["visits"].sum()) == c["n"] * c["T"] - ref.n_left_out
    b.close()


# ---- W: the grid-stride loop of the act kernels wraps ---------------------------------------------------------------------------------
@pytest.mark.parametrize("learner", LEARNERS)
def test_run_on_more_lanes_than_two_full_grids(host, learner):
    import torch
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    c = grid_wrap_case(cus)
    if c["n"] > MAX_LANES:
        pytest.skip("%d compute units: two full grids are %d lanes, a learner takes at most 2^22" % (cus, c["n"]))
    assert c["n"] > 8 * 256 * cus                              # a launch is capped at 8 workgroups of 256 per compute unit
    o, ref, st, m = reference(learner, "W", host, compute_units=cus)
    assert m["frozen"].sum() == 52 and not m["frozen"][:2 * 8 * 256 * cus].any()       # any_frozen: the third iteration alone
    assert ref.n_left_out == 52 * c["T"] and ref.n_truncated > 0 and ref.n_terminated > 0 and int(o.hist.sum()) >= c["n"] - 52
    b, q = device_run(learner, c, [c["T"]], st)
    assert_equals_reference(learner, b, q, o, ref, misuse=SoccerBatch.MISUSE_FROZEN)
    b.close()


# ---- U: update() where the reduce kernel wraps and where the integer sums are largest -----------------------------------------------
def _one_cell(n, nS, reward):
    """n transitions of the cell (17, 3, 1): reward 0 and a live next state, or a terminal reward"""
    term = reward != 0
    return (np.full(n, 17), np.full(n, 3), np.full(n, 1), np.full(n, reward), np.full(n, int(term), np.uint8),
            np.full(n, 0 if term else nS - 2))


def _updates_equal(host, learner, batches, **over):
    b = SoccerBatch(8, 5, 4, 0.0, seed=1, autoreset=True)
    q = new_learner(b, learner, **over)
    ref = new_restatement(learner, b.nS, host, **over)
    for batch in batches(b.nS):
        q.update(*batch); ref.update(*batch)
        assert_read_equal(learner, q.read(), ref.state())
    assert b.misuse() == 0
    b.close()
    return ref


@pytest.mark.parametrize("learner", LEARNERS)
def test_update_on_more_transitions_than_one_grid(host, learner):
    import torch
    n = 2 ** 21 + 259
    assert 8 * 256 * int(torch.cuda.get_device_properties(0).multi_processor_count) < n <= MAX_LANES
    rng = np.random.default_rng(1994)
    _updates_equal(host, learner, lambda nS: (_random_batch(np.random.default_rng(7), nS, 20000), _random_batch(rng, nS, n)),
                   alpha=0.75, decay=0.9, q_init=0.5)


@pytest.mark.parametrize("q_init", [1.0, -1.0])
@pytest.mark.parametrize("learner", LEARNERS)
def test_update_with_the_largest_sum_of_values(host, learner, q_init):
    """2^22 samples of |V| = 1 in one cell: the sum is +-2^62, the last that fits int64 with room, and the update is still exact"""
    ref = _updates_equal(host, learner, lambda nS: (_one_cell(MAX_LANES, nS, 0),), alpha=0.75, q_init=q_init)
    s = ref.state()
    got = s["Q"][17, 3, 1] if learner == "minimax_q" else s["Q_a"][17, 3]
    assert got == q_init + 0.75 * ((0.0 + GAMMA * (q_init * 2.0 ** 62 * 2.0 ** -40) / 2.0 ** 22) - q_init)
    assert int(s["visits"][17, 16]) == MAX_LANES


@pytest.mark.parametrize("learner", LEARNERS)
def test_update_with_the_largest_sum_of_rewards(host, learner):
    """2^22 terminated samples in one cell, all of reward +1, then all of reward -1: the reward sum is +-2^22"""
    ref = _updates_equal(host, learner, lambda nS: (_one_cell(MAX_LANES, nS, 1), _one_cell(MAX_LANES, nS, -1)), alpha=0.75, decay=0.5,
                         q_init=0.5)
    s = ref.state()
    got = s["Q"][17, 3, 1] if learner == "minimax_q" else s["Q_a"][17, 3]
    first = 0.5 + 0.75 * (1.0 - 0.5)
    assert got == first + 0.375 * (-1.0 - first) and int(s["visits"][17, 16]) == 2 * MAX_LANES


# ---- L: more than 48 KB of dynamic LDS ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("learner", LEARNERS)
def test_act_kernels_with_more_than_48_kb_of_lds(host, learner):
    c = CASES["L"]
    o, ref = reference(learner, "L", host)[:2]
    assert ref.n_terminated > 0
    b, q = device_run(learner, c, [c["T"]])
    assert b.nS == 12641
    assert_equals_reference(learner, b, q, o, ref)
    # the act kernels are launched with the handle's table bytes, which is what its per-lane rollout kernel is launched with:
    # a one-step rollout that has to take that kernel (a reward stream no vector store can write) reports them
    rew = b.alloc(c["n"] + 8, np.int8)
    b.rollout(1, sample_actions=True, reward=rew.ptr + 1, out_stride=c["n"] + 4)
    sh = b.rollout_shape()
    assert sh["kernel"] == _lib.ROLLOUT_PER_LANE and sh["dynamic_lds_bytes"] > 48 * 1024
    assert sh["dynamic_lds_bytes"] > (o.W * o.H) ** 2 * 4      # the observation table is staged in it
    b.close()


# ---- G: the observation table in global memory ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("learner", LEARNERS)
def test_act_kernels_with_the_observation_table_in_global_memory(host, learner):
    """12x14: learner_act_kernel / q_act_kernel / phc_act_kernel with LUT_LDS = false, which stage the move table alone"""
    c = CASES["G"]
    o, ref = reference(learner, "G", host)[:2]
    assert ref.n_terminated > 0 and ref.n_truncated > 0
    b, q = device_run(learner, c, [c["T"]])
    assert b.nS == 56113
    assert_equals_reference(learner, b, q, o, ref)
    rew = b.alloc(c["n"] + 8, np.int8)
    b.rollout(1, sample_actions=True, reward=rew.ptr + 1, out_stride=c["n"] + 4)     # as in L: what the act kernels are launched with
    sh = b.rollout_shape()
    assert sh["kernel"] == _lib.ROLLOUT_PER_LANE and 0 < sh["dynamic_lds_bytes"] < (o.W * o.H) ** 2 * 4
    assert sh["dynamic_lds_bytes"] == (2 * o.W * o.H * 5 + 16) * 4
    b.close()


# ---- O: lane ids beyond 2^32 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("learner", LEARNERS)
def test_lane_offset_carries_lane_ids_across_2_32(host, learner):
    c = CASES["O"]
    o, ref = reference(learner, "O", host)[:2]
    assert c["lane_offset"] < 2 ** 32 < c["lane_offset"] + c["n"] and ref.n_truncated > ref.n_terminated > 0
    b, q = device_run(learner, c, [c["T"]])
    assert_equals_reference(learner, b, q, o, ref)
    b0, q0 = device_run(learner, CASES["O at offset 0"], [c["T"]])
    key = "Q" if learner == "minimax_q" else "Q_a"
    assert q0.read()[key].tobytes() != q.read()[key].tobytes()
    assert (b0.get_state()["row_a"] != b.get_state()["row_a"]).any()
    b.close(); b0.close()
