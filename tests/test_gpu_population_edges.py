"""-m gpu: the three per-lane learner populations (Q-learners, WoLF-PHC, minimax-Q; pop_run_kernel, phc_pop_run_kernel,
mq_pop_run_kernel) against their numpy restatements, bit for bit, away from the plain lanes their own suites run: every
transition truncating (T1), frozen, goal-parked and nearly-out-of-time lanes beside plain ones in one launch (S, S250), a lane
offset that carries lane ids across 2^32 (O), more than 48 KB of dynamic LDS (L), the observation table left in global memory
(G) and a member loop that wraps (W: SOCCER_POP_GRID_BLOCKS, SOCCER_MQ_POP_WAVES).  The cases are defined in
tests/test_population_edges_np.py, which also shows without a GPU that each reaches its path.  No tolerances."""
import os
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch, _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_q_learning import assert_batches_equal, assert_state_equal  # noqa: E402
from test_matrix_game_host import build_games_host  # noqa: E402
from test_population_edges_np import (CASES, CONFIGS, G0_KINDS, GAMMA, KINDS, KW, LDS_TABLE_LIMIT, PER_MEMBER, SEED, TABLES, W_ENV,  # noqa: E402
                                      W_GRID, assert_read_equal, case_of, counts, population_args, reference, reference_g0,
                                      reference_w_then_update)

pytestmark = pytest.mark.gpu

METHOD = {"q": "q_population", "wolf": "wolf_population", "minimax_q": "minimax_q_population"}
FACTOR = {"alpha": "decay", "dscale": "delta_decay"}           # what a per-member value is multiplied by every step


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_games_host(tmp_path_factory.mktemp("games_pop_edges_gpu"))


def new_batch(c):
    return SoccerBatch(c["n"], c["w"], c["h"], c["slip"], seed=SEED, autoreset=True, max_steps=c["max_steps"],
                       lane_offset=c.get("lane_offset", 0))


def new_population(b, kind, config="learn"):
    return getattr(b, METHOD[kind])(GAMMA, **population_args(kind, config, b.n, b.nS))


def device_run(kind, c, parts, st=None, config="learn", start=None):
    """a fresh handle and population (loaded where the case starts from a loaded state): reset, the case's special lanes, then
    run() part by part"""
    b = new_batch(c)
    q = new_population(b, kind, config)
    if start is not None:
        q.load(**start)
    b.reset()
    if st is not None:
        b.set_state(**st)
    for t in parts:
        q.run(t)
    return b, q


def assert_equals_reference(kind, b, q, o, ref, frozen=False):
    """the whole read(), the state streams, the tick, the episode histogram, the misuse word, steps and the per-member values"""
    got = q.read()
    assert_read_equal(kind, got, ref.state())
    assert_state_equal(b, o)
    assert b.tick == o.tick == ref.steps + 1
    hist, misuse = b.stats()
    np.testing.assert_array_equal(hist, o.hist)
    assert misuse == (SoccerBatch.MISUSE_FROZEN if frozen else 0) and (o.misuse > 0) == frozen
    assert hist.sum() > 0 and q.steps == ref.steps == got["steps"]
    for k in PER_MEMBER[kind]:
        assert getattr(q, k).tobytes() == getattr(ref, k).tobytes(), k
    if kind == "wolf":
        np.testing.assert_array_equal(got["updates"], ref.updates)
    mid = b.n // 2                                              # a range is the slice
    part, want = q.read(mid, 1), ref.state(mid, 1)
    for k in TABLES[kind] + PER_MEMBER[kind]:
        assert np.asarray(part[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    return got


def assert_same_populations(kind, q1, q2):
    r1, r2 = q1.read(), q2.read()
    for k in TABLES[kind] + PER_MEMBER[kind]:
        assert np.asarray(r1[k]).tobytes() == np.asarray(r2[k]).tobytes(), k
    assert r1["steps"] == r2["steps"]


def run_with_frozen_members(kind, name, host, config):
    """a case with frozen lanes: beside the comparison, a frozen member's lane is unchanged byte for byte, its tables are a
    freshly created population's (where the case starts from a loaded state: what was loaded and solved from it), and its alpha
    (WoLF: its dscale too) has advanced T times"""
    c = case_of(kind, name)
    o, ref, st, m = reference(kind, name, host, config)
    print("%s %s %s: %s" % (kind, config, name, counts(ref)))
    frozen = m["frozen"]
    lo = int(np.flatnonzero(frozen)[0])
    b = new_batch(c)
    q = new_population(b, kind, config)
    if ref.start is not None:
        q.load(**ref.start)
    fresh = q.read(lo)                                          # (W: the ragged third grid alone)
    b.reset()
    b.set_state(**st)
    before = b.get_state()
    q.run(c["T"])
    got = assert_equals_reference(kind, b, q, o, ref, frozen=True)
    after = b.get_state()
    for k in before:
        assert after[k][frozen].tobytes() == before[k][frozen].tobytes(), k
    for k in TABLES[kind]:
        assert got[k][lo:][frozen[lo:]].tobytes() == fresh[k][frozen[lo:]].tobytes(), k
    key = "Q" if kind == "minimax_q" else "Q_a"
    assert (got[key][lo:][~frozen[lo:]] != fresh[key][~frozen[lo:]]).any(axis=tuple(range(1, fresh[key].ndim))).all()      # (every other member learned)
    for k in PER_MEMBER[kind]:
        want = fresh[k].copy()
        for _ in range(c["T"]):
            want = want * KW[kind][FACTOR[k]]
        assert got[k][lo:].tobytes() == want.tobytes() and (want != fresh[k]).all(), k
    return b, q


# ---- T1: every transition truncates ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("kind", KINDS)
def test_with_max_steps_1_every_step_reloads_the_rows_and_bootstraps_from_final_obs(host, kind, config, monkeypatch):
    c = CASES["T1"]
    o, ref = reference(kind, "T1", host, config)[:2]
    assert (ref.n_truncated_only, ref.n_terminated, ref.n_left_out) == (c["n"] * c["T"], 0, 0)
    b, q = device_run(kind, c, [c["T"]], config=config)
    assert_equals_reference(kind, b, q, o, ref)
    # in two runs, and as one run of launches of seven steps: the single launch's result and batch state
    b2, q2 = device_run(kind, c, [13, 27], config=config)
    monkeypatch.setenv("SOCCER_POP_LAUNCH_STEPS", "7")
    b3, q3 = device_run(kind, c, [c["T"]], config=config)
    monkeypatch.delenv("SOCCER_POP_LAUNCH_STEPS")
    for bx, qx in ((b2, q2), (b3, q3)):
        assert_same_populations(kind, qx, q)
        assert_batches_equal(bx, b)
        assert bx.misuse() == 0
    b.close(); b2.close(); b3.close()


# ---- S, S250: special lanes beside plain ones ------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("kind", KINDS)
def test_frozen_parked_and_late_lanes_beside_plain_ones(host, kind, config, monkeypatch):
    c = CASES["S"]
    o, ref, st, m = reference(kind, "S", host, config)
    assert ref.n_left_out == 52 * c["T"] + 30 and ref.n_truncated_only >= 16 and ref.n_terminated > 0
    b, q = run_with_frozen_members(kind, "S", host, config)
    # in two runs, and as one run of launches of seven steps: the single launch's result and batch state
    b2, q2 = device_run(kind, c, [5, 7], st, config, ref.start)
    monkeypatch.setenv("SOCCER_POP_LAUNCH_STEPS", "7")
    b3, q3 = device_run(kind, c, [c["T"]], st, config, ref.start)
    monkeypatch.delenv("SOCCER_POP_LAUNCH_STEPS")
    for bx, qx in ((b2, q2), (b3, q3)):
        assert_same_populations(kind, qx, q)
        assert_batches_equal(bx, b)
        assert bx.misuse() == SoccerBatch.MISUSE_FROZEN
    b.close(); b2.close(); b3.close()


@pytest.mark.parametrize("kind", KINDS)
def test_special_lanes_with_max_steps_near_the_end_of_uint8(host, kind):
    o, ref, st, m = reference(kind, "S250", host)
    assert int(st["t"].max()) == 249 and ref.n_left_out == 52 * 12 + 30 and ref.n_truncated_only >= 16
    b, q = run_with_frozen_members(kind, "S250", host, "learn")
    b.close()


# ---- W: the member loop of the run kernel wraps -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_run_and_update_on_more_members_than_two_full_grids(host, kind, monkeypatch):
    """That the variable took effect cannot be seen from here: by design it changes no result, and nothing the ABI reports
    names a population's grid.  If it were ignored (misspelt, read too late) this test would pass on one grid, as the test of
    SOCCER_MQ_POP_WAVES in tests/test_gpu_minimax_q_population.py would.  What holds it is the code: pop_grid_blocks_env and
    pop_grid in csrc/soccer_learners.hip, read beside SOCCER_POP_LAUNCH_STEPS."""
    c = case_of(kind, "W")
    o, ref, st, m = reference(kind, "W", host)
    assert c["n"] > 2 * W_GRID[kind] and not m["frozen"][:2 * W_GRID[kind]].any()       # any_frozen: the third iteration alone
    assert ref.n_left_out == int(m["frozen"].sum()) * c["T"] > 0
    monkeypatch.setenv(*W_ENV[kind])                            # read at creation
    b, q = run_with_frozen_members(kind, "W", host, "learn")
    monkeypatch.delenv(W_ENV[kind][0])
    # update() goes through the same capped grid: one transition per member, the member loop of the update kernel wraps too
    ref2, batch = reference_w_then_update(kind, host)
    q.update(*batch)
    assert_read_equal(kind, q.read(), ref2.state())
    assert q.steps == c["T"] + 1 and b.misuse() == SoccerBatch.MISUSE_FROZEN       # (the run's flag is sticky; update() raised none)
    b.close()


# ---- O: lane ids beyond 2^32 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_lane_offset_carries_lane_ids_across_2_32(host, kind):
    c = CASES["O"]
    o, ref = reference(kind, "O", host)[:2]
    assert c["lane_offset"] < 2 ** 32 < c["lane_offset"] + c["n"] and ref.n_truncated_only > 0 and ref.n_terminated > 0
    b, q = device_run(kind, c, [c["T"]])
    assert_equals_reference(kind, b, q, o, ref)
    o0, ref0 = reference(kind, "O0", host)[:2]
    b0, q0 = device_run(kind, CASES["O0"], [c["T"]])
    assert_equals_reference(kind, b0, q0, o0, ref0)
    key = "Q" if kind == "minimax_q" else "Q_a"
    assert q0.read()[key].tobytes() != q.read()[key].tobytes()
    s, s0 = b.get_state(), b0.get_state()
    assert any((s[k] != s0[k]).any() for k in ("row_a", "col_a", "row_b", "col_b"))
    assert (s["row_a"] != s0["row_a"]).any()
    b.close(); b0.close()


# ---- L: more than 48 KB of dynamic LDS ------------------------------------------------------------------------------------------
def per_lane_rollout_shape(b):
    """the run kernels of the Q and WoLF populations are launched with the handle's table bytes, which is what its per-lane
    rollout kernel is launched with: a one-step rollout that has to take that kernel (a reward stream no vector store can
    write) reports them: the move table, and the observation table where the kernels stage it (LUT_LDS)"""
    rew = b.alloc(b.n + 8, np.int8)
    b.rollout(1, sample_actions=True, reward=rew.ptr + 1, out_stride=b.n + 4)
    sh = b.rollout_shape()
    assert sh["kernel"] == _lib.ROLLOUT_PER_LANE
    return sh


@pytest.mark.parametrize("kind", KINDS)
def test_run_kernels_with_more_than_48_kb_of_lds(host, kind):
    c = CASES["L"]
    o, ref = reference(kind, "L", host)[:2]
    assert ref.n_terminated > 0
    b, q = device_run(kind, c, [c["T"]])
    assert b.nS == 12641
    assert c["n"] > (32 << 20) // (b.nS * 80)                  # read() crosses the host staging block of every kind (Q's rows are the smallest)
    assert_equals_reference(kind, b, q, o, ref)
    sh = per_lane_rollout_shape(b)
    print("L: %d bytes of dynamic LDS, the observation table is %d bytes" % (sh["dynamic_lds_bytes"], 2 * o.tables()[0].size))
    assert sh["dynamic_lds_bytes"] > 48 * 1024
    assert sh["dynamic_lds_bytes"] > 2 * o.tables()[0].size == (o.W * o.H) ** 2 * 4      # the observation table is staged in it: LUT_LDS
    b.close()


# ---- G: the observation table stays in global memory ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_run_kernels_with_the_observation_table_in_global_memory(host, kind):
    c = CASES["G"]
    o, ref = reference(kind, "G", host)[:2]
    assert 2 * o.tables()[0].size > LDS_TABLE_LIMIT and ref.n_terminated > 0 and ref.n_truncated_only > 0
    b, q = device_run(kind, c, [c["T"]])
    assert b.nS == 56113
    assert_equals_reference(kind, b, q, o, ref)
    sh = per_lane_rollout_shape(b)
    print("G: %d bytes of dynamic LDS, the observation table is %d bytes" % (sh["dynamic_lds_bytes"], 2 * o.tables()[0].size))
    # the move table alone is staged: the observation table is read from global memory (LUT_LDS = false)
    assert 0 < sh["dynamic_lds_bytes"] < 2 * o.tables()[0].size and sh["dynamic_lds_bytes"] + 2 * o.tables()[0].size > LDS_TABLE_LIMIT
    q.close()                                                  # before the handle: a failure shows up here, not in the next test
    assert b.misuse() == 0
    b.close()


@pytest.mark.parametrize("kind", [k for k in KINDS if k in G0_KINDS])
def test_run_kernels_with_the_observation_table_in_global_memory_without_slip(kind):
    """G0: the <SLIP = false, LUT_LDS = false> run kernels of the populations whose members are threads (minimax-Q's takes no
    LUT_LDS); the opponent-modelling and the league populations run the case in their own suites"""
    c = CASES["G0"]
    o, ref = reference_g0(kind)
    assert 2 * o.tables()[0].size > LDS_TABLE_LIMIT and c["slip"] == 0.0
    assert ref.n_terminated > 0 and ref.n_truncated_only > 0 and ref.n_same > 0
    b, q = device_run(kind, c, [c["T"]])
    assert b.nS == 56113
    assert_equals_reference(kind, b, q, o, ref)
    q.close()
    assert b.misuse() == 0
    b.close()
