"""-m gpu: the three per-lane learner populations (Q-learners, WoLF-PHC, minimax-Q; pop_run_kernel, phc_pop_run_kernel,
mq_pop_run_kernel) against their numpy restatements, bit for bit, away from the plain lanes their own suites run: every
transition truncating (T1), frozen, goal-parked and nearly-out-of-time lanes beside plain ones in one launch (S, S250), a lane
offset that carries lane ids across 2^32 (O), more than 48 KB of dynamic LDS (L), the observation table left in global memory
(G) and a member loop that wraps (W: SOCCER_POP_GRID_BLOCKS, SOCCER_MQ_POP_WAVES).  The cases are defined in
tests/test_population_edges_np.py, which also shows without a GPU that each reaches its path.  No tolerances.

The same cases (G apart, which their own suites run) hold the two run kernels that carry more than rows: om_pop_run_kernel
(the opponent-modelling population: the pair (g_A[s], g_B[s])) and pop_league_run_kernel (the Q population against a league
that plays A or B: a pick beside the rows, compared through picks()).  Then the league at the end of its draw's counter
range (H: a run that ends exactly at tick 2^62, the refusal beyond it, a tick whose low word carries), and the device's
om_derive at its edges, which read() cannot show since it derives V and pi in numpy: crafted rows are loaded, and what the
device derived from them is seen in the cell an update() moves and in the action a greedy step takes."""
import os
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch, _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_q_learning import assert_batches_equal, assert_state_equal  # noqa: E402
from test_matrix_game_host import build_games_host  # noqa: E402
from league_np import league_pick  # noqa: E402
from om_population_np import assert_om_population_equal  # noqa: E402
from philox_np import lane_words  # noqa: E402
from test_population_edges_np import (ALL_KINDS, CASES, CONFIGS, D_BIG, D_KW, D_N, G0_KINDS, GAMMA, H_SLIPS, H_TICKS, KINDS, KW,  # noqa: E402
                                      LDS_TABLE_LIMIT, LEAGUE_PLAYER, PER_MEMBER, SEED, TABLES, W_ENV, W_GRID, assert_read_equal,
                                      case_of, counts, derive_case, new_oracle, new_restatement, population_args, reference,
                                      reference_g0, reference_h, reference_w_then_update)

pytestmark = pytest.mark.gpu

METHOD = {"q": "q_population", "wolf": "wolf_population", "minimax_q": "minimax_q_population", "om": "om_population",
          "league_a": "q_population", "league_b": "q_population"}
FACTOR = {"alpha": "decay", "dscale": "delta_decay"}           # what a per-member value is multiplied by every step


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_games_host(tmp_path_factory.mktemp("games_pop_edges_gpu"))


def new_batch(c):
    return SoccerBatch(c["n"], c["w"], c["h"], c["slip"], seed=SEED, autoreset=True, max_steps=c["max_steps"],
                       lane_offset=c.get("lane_offset", 0))


def new_population(b, kind, config="learn"):
    return getattr(b, METHOD[kind])(GAMMA, **population_args(kind, config, b.n, b.nS))


def read_all(kind, q, first=0, count=None):
    """read(), for a league with its picks() under "pick": what the restatement's state() holds"""
    r = q.read(first, count)
    if kind in LEAGUE_PLAYER:
        r["pick"] = q.picks(first, count)
    return r


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
    """the whole read() (a league: and its picks), the state streams, the tick, the episode histogram, the misuse word, steps and
    the per-member values"""
    got = read_all(kind, q)
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
    part, want = read_all(kind, q, mid, 1), ref.state(mid, 1)
    for k in TABLES[kind] + PER_MEMBER[kind]:
        assert np.asarray(part[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    return got


def assert_same_populations(kind, q1, q2):
    r1, r2 = read_all(kind, q1), read_all(kind, q2)
    for k in TABLES[kind] + PER_MEMBER[kind]:
        assert np.asarray(r1[k]).tobytes() == np.asarray(r2[k]).tobytes(), k
    assert r1["steps"] == r2["steps"]


def run_with_frozen_members(kind, name, host, config):
    """a case with frozen lanes: beside the comparison, a frozen member's lane is unchanged byte for byte, its tables are a
    freshly created population's (where the case starts from a loaded state: what was loaded and solved from it), and its alpha
    (WoLF: its dscale too) has advanced T times.  The opponent-modelling kind: its counts among the tables, still zero.  A league:
    its pick is what the first run step drew for its lane, and nothing cleared or redrew it."""
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
    tick0 = b.tick                                              # the tick of the first run step
    q.run(c["T"])
    got = assert_equals_reference(kind, b, q, o, ref, frozen=True)
    after = b.get_state()
    for k in before:
        assert after[k][frozen].tobytes() == before[k][frozen].tobytes(), k
    for k in TABLES[kind]:
        if k != "pick":
            assert got[k][lo:][frozen[lo:]].tobytes() == fresh[k][frozen[lo:]].tobytes(), k
    if kind == "om":
        assert not got["C_a"][frozen].any() and not got["C_b"][frozen].any()
    if kind in LEAGUE_PLAYER:
        ids = c.get("lane_offset", 0) + np.flatnonzero(frozen)
        first = league_pick(ref.T, lane_words(SEED, ids, 2 ** 62 + tick0, purpose=1))
        assert got["pick"][frozen].tolist() == first.tolist() and set(first.tolist()) == {0, 1, 2} and tick0 > 0
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
@pytest.mark.parametrize("kind", ALL_KINDS)
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
@pytest.mark.parametrize("kind", ALL_KINDS)
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


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_special_lanes_with_max_steps_near_the_end_of_uint8(host, kind):
    o, ref, st, m = reference(kind, "S250", host)
    assert int(st["t"].max()) == 249 and ref.n_left_out == 52 * 12 + 30 and ref.n_truncated_only >= 16
    b, q = run_with_frozen_members(kind, "S250", host, "learn")
    b.close()


# ---- W: the member loop of the run kernel wraps -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ALL_KINDS)
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
    picks = q.picks() if kind in LEAGUE_PLAYER else None
    q.update(*batch)
    assert_read_equal(kind, read_all(kind, q), ref2.state())
    if kind in LEAGUE_PLAYER:                                   # update() leaves every pick alone
        assert q.picks().tolist() == picks.tolist() and (picks >= 0).any() and (picks == -1).any()
    assert q.steps == c["T"] + 1 and b.misuse() == SoccerBatch.MISUSE_FROZEN       # (the run's flag is sticky; update() raised none)
    b.close()


# ---- O: lane ids beyond 2^32 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ALL_KINDS)
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


@pytest.mark.parametrize("kind", ALL_KINDS)
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


# ---- H: the league's draw at counter 2^62 + tick, to the end of its range ------------------------------------------------------------
def set_tick(b, tick):
    b._check(b.lib.soccer_set_tick(b.h, tick))


def league_at_tick(slip, tick):
    """case H's handle and league population (the league plays B), reset, the tick then set"""
    b = new_batch(dict(CASES["H"], slip=slip))
    q = new_population(b, "league_b")
    b.reset()
    set_tick(b, tick)
    return b, q


def assert_equals_reference_at_tick(b, q, o, ref):
    """assert_equals_reference where the tick is not steps + 1"""
    assert_read_equal("league_b", read_all("league_b", q), ref.state())
    assert_state_equal(b, o)
    assert b.tick == o.tick
    hist, misuse = b.stats()
    np.testing.assert_array_equal(hist, o.hist)
    assert misuse == 0 and hist.sum() > 0 and q.steps == ref.steps and q.alpha.tobytes() == ref.alpha.tobytes()


def everything(b, q):
    hist, misuse = b.stats()
    return read_all("league_b", q), b.get_state(), b.tick, hist.tolist(), misuse


def assert_nothing_changed(b, q, before):
    r, s, tick, hist, misuse = everything(b, q)
    assert_read_equal("league_b", r, before[0])
    for k in s:
        np.testing.assert_array_equal(s[k], before[1][k], err_msg=k)
    assert (tick, hist, misuse) == before[2:]


@pytest.mark.parametrize("tick", H_TICKS, ids=["2^62-20", "2^32-7"])
@pytest.mark.parametrize("slip", H_SLIPS)
def test_league_run_at_a_high_tick(slip, tick):
    c = CASES["H"]
    o, ref = reference_h(slip, tick)
    assert ref.n_terminated > 0 and ref.n_truncated_only > 100 and ref.n_redraws > 100 and ref.seen == {0, 1, 2}
    b, q = league_at_tick(slip, tick)
    q.run(c["T"])
    assert b.tick == tick + c["T"] and (tick + c["T"] == 2 ** 62 or tick < 2 ** 32 < tick + c["T"])
    assert_equals_reference_at_tick(b, q, o, ref)
    ref1 = reference_h(slip, None)[1]                           # the run at tick 1 is another
    assert q.read()["Q_a"].tobytes() != ref1.state()["Q_a"].tobytes()
    b.close()


REFUSAL = r"soccer_q_population_run: a league population's run may not cross tick 2\^62"


def test_a_league_run_may_end_at_tick_2_62_and_not_cross_it():
    c, slip = CASES["H"], 0.2
    o, ref = reference_h(slip, 2 ** 62 - c["T"])
    b, q = league_at_tick(slip, 2 ** 62 - c["T"])
    q.run(c["T"])
    assert b.tick == 2 ** 62
    assert_equals_reference_at_tick(b, q, o, ref)
    before = everything(b, q)
    with pytest.raises(AssertionError, match=REFUSAL):
        q.run(1)
    assert_nothing_changed(b, q, before)
    # a population without a league draws nothing at 2^62 + tick: at the same tick it runs
    b2 = new_batch(dict(c, slip=slip))
    p = b2.q_population(GAMMA, **KW["q"])
    b2.reset()
    set_tick(b2, 2 ** 62)
    p.run(1)
    assert p.steps == 1 and b2.tick == 2 ** 62 + 1 and b2.misuse() == 0
    b.close(); b2.close()
    # five steps before the end: six are refused and change nothing, five run
    b, q = league_at_tick(slip, 2 ** 62 - 5)
    before = everything(b, q)
    with pytest.raises(AssertionError, match=REFUSAL):
        q.run(6)
    assert_nothing_changed(b, q, before)
    q.run(5)
    o = new_oracle(dict(c, slip=slip))
    obs = o.reset()
    o.tick = 2 ** 62 - 5
    ref = new_restatement("league_b", "learn", c["n"], o.nS, None)
    ref.run(o, obs, 5)
    assert b.tick == 2 ** 62 and ref.n_redraws > 0
    assert_equals_reference_at_tick(b, q, o, ref)
    b.close()


# ---- D: what the device derives from crafted rows ---------------------------------------------------------------------------------------
def test_derived_values_on_the_device_at_the_edges_of_their_definition():
    """om_derive after load() (om_pop_derive_kernel) and after an update (om_learn), for both players, on rows with n = 0 beside
    a non-constant Q, an exact tie, counts (3, 0, 0, 0, 1), counts beyond 2^53 over ones and over minus ones, and plain rows
    (tests/test_population_edges_np.py, case D).  V shows in the cell update() moves when next_obs is such a row, g in the
    action a lane on such a row takes with explor = 0, which the cell and the count of the run's update name.  (Of the clamp
    itself the bootstrap shows nothing: 1 + 2^-51 and 1 are the same multiple of 2^-40.  What it shows there is the sum with
    weights of 2^53 and the counts' conversion.)"""
    d = derive_case()
    c, S, n = d["c"], d["S"], D_N
    b = new_batch(c)
    q = b.om_population(GAMMA, **D_KW)
    q.load(**d["start"])
    assert_om_population_equal(q.read(), d["loaded"])
    b.reset()
    q.update(*d["batch"])
    got = q.read()
    assert_om_population_equal(got, d["updated"])
    assert b.misuse() == 0 and got["steps"] == 1
    big = [int(x) for x in got["C_a"][got["C_a"] > 2 ** 53]] + [int(x) for x in got["C_b"][got["C_b"] > 2 ** 53]]
    assert D_BIG in big and D_BIG + 1 in big and set(big) == {D_BIG, D_BIG + 1}        # exact integers, odd ones among them
    b.set_state(**d["place"])
    q.run(1)
    ran = q.read()
    assert_om_population_equal(ran, d["ran"])
    assert_state_equal(b, d["oracle"])
    assert b.tick == d["oracle"].tick == 2 and b.misuse() == 0
    np.testing.assert_array_equal(b.stats()[0], d["oracle"].hist)
    for C_own, other in (("C_a", 1), ("C_b", 0)):               # the pair of actions: each count that rose names the other's
        rose = (ran[C_own] - got[C_own])[np.arange(n), S[d["k_run"]]]
        assert (rose.sum(1) == 1).all() and (rose.argmax(1) == d["acts"][other]).all()
    assert ran["steps"] == 2 and q.alpha.tobytes() == d["ref"].alpha.tobytes()
    b.close()
