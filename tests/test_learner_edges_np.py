"""The settings in which tests/test_gpu_learner_edges.py holds the three on-device learners to their numpy restatements, defined
once, and what can be said about them without a GPU: every case reaches the path it is for (truncated, terminated or left-out
transitions, counted by the restatements' run()), the restatement tells a truncated transition from a terminated one and
final_obs from obs, WoLF-PHC takes every branch of its policy step under truncation, and the lane filter leaves frozen and
goal-parked lanes out.  This guards the yardstick where there is no GPU."""
import os
import sys

import numpy as np
import pytest

from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import minimax_q_np as mq_np  # noqa: E402
import q_learning_np as ql_np  # noqa: E402
import wolf_phc_np as phc_np  # noqa: E402
from q_learning_np import observations  # noqa: E402
from test_matrix_game_host import build_games_host  # noqa: E402

GAMMA, SEED = 0.9, 1994
LEARNERS = ("minimax_q", "q_learning", "wolf_phc")
# as in the run tests of each learner: minimax-Q against itself, greedy / greedy, learn / learn with decaying deltas
KW = {"minimax_q": dict(explor=0.2, decay=0.99, opponent="self"),
      "q_learning": dict(explor=0.2, decay=0.99),
      "wolf_phc": dict(explor=0.2, decay=0.99, delta_win=0.1, delta_lose=0.4, delta_decay=0.98)}
MAX_LANES = 2 ** 22

# name -> width, height, slip, lanes, max_steps, learner steps, lane offset, how lanes are prepared after reset()
CASES = {
    "T": dict(w=5, h=4, slip=0.2, n=8192 + 3, max_steps=6, T=40),
    "T every transition truncates": dict(w=5, h=4, slip=0.0, n=4096 + 3, max_steps=1, T=10),
    "S": dict(w=5, h=4, slip=0.2, n=4096 + 3, max_steps=9, T=12, special="mixed"),
    "S uint8 end of t": dict(w=5, h=4, slip=0.2, n=4096 + 3, max_steps=250, T=12, special="mixed"),
    "L": dict(w=5, h=16, slip=0.2, n=8192 + 3, max_steps=100, T=30),
    "O": dict(w=5, h=4, slip=0.2, n=4096 + 3, max_steps=6, T=20, lane_offset=2 ** 32 - 4096),
    # the pitch, slip and max_steps of the populations' G (tests/test_population_edges_np.py): the observation table does not fit LDS
    "G": dict(w=12, h=14, slip=0.2, n=4096 + 3, max_steps=7, T=16),
}
# the same handle as O at offset 0: what O must differ from
CASES["O at offset 0"] = dict(CASES["O"], lane_offset=0)


def grid_wrap_case(compute_units):
    """W: more lanes than twice the launch cap of 8 workgroups of 256 threads per compute unit, so that every grid-stride loop
    of the act kernels runs two full iterations and 259 lanes of a third; every fifth of those 259 is frozen."""
    return dict(w=5, h=4, slip=0.2, n=2 * 8 * 256 * int(compute_units) + 259, max_steps=3, T=3, special="frozen tail")


def case_of(name, compute_units=None):
    return grid_wrap_case(compute_units) if name == "W" else CASES[name]


def new_restatement(learner, nS, host, **over):
    kw = dict(KW[learner]); kw.update(over)
    if learner == "minimax_q":
        return mq_np.MinimaxQNumpy(host, nS, GAMMA, **kw)
    if learner == "q_learning":
        return ql_np.QLearningNumpy(nS, GAMMA, **kw)
    return phc_np.WolfPHCNumpy(nS, GAMMA, **kw)


def assert_read_equal(learner, got, want):
    {"minimax_q": mq_np.assert_learner_equal, "q_learning": ql_np.assert_learner_equal, "wolf_phc": phc_np.assert_phc_equal}[learner](got, want)


def new_oracle(c):
    return Oracle(c["w"], c["h"], c["slip"], n=c["n"], seed=SEED, lane_offset=c.get("lane_offset", 0), autoreset=True,
                  max_steps=c["max_steps"])


def a_goal_tuple(orc):
    """(row_a, col_a, row_b, col_b, poss) of the first goal tuple of the oracle's tables"""
    f = int(np.flatnonzero(orc.tables()[1] == 2)[0])
    p = f & 1; r = f >> 1
    yb = r % orc.W; r //= orc.W; xb = r % orc.H; r //= orc.H; ya = r % orc.W; xa = r // orc.W
    return xa, ya, xb, yb, p


def special_state(c, orc):
    """the arguments of set_state (the oracle's and the handle's alike) that turn the lanes of a freshly reset oracle into the
    case's mix, and masks of who is what; None for a case of plain lanes.  'frozen tail': every fifth of the last c["tail"] lanes
    (259 where the case names none) is frozen."""
    kind = c.get("special")
    if kind is None:
        return None, {}
    n = c["n"]
    st = dict(row_a=orc.row_a.copy(), col_a=orc.col_a.copy(), row_b=orc.row_b.copy(), col_b=orc.col_b.copy(),
              poss=(orc.poss & 1).astype(np.uint8), t=orc.t.copy(), needs_reset=((orc.poss >> 1) & 1).astype(np.uint8))
    frozen = np.zeros(n, bool); parked = np.zeros(n, bool); late = np.zeros(n, bool)
    if kind == "frozen tail":
        frozen[n - c.get("tail", 259)::5] = True
    else:
        frozen[::5] = True
        rest = np.flatnonzero(~frozen)
        parked[rest[1::7]] = True
        rest = np.flatnonzero(~frozen & ~parked)
        late[rest[2::11]] = True
        for k, v in zip(("row_a", "col_a", "row_b", "col_b", "poss"), a_goal_tuple(orc)):
            st[k][parked] = v
        st["t"][late] = c["max_steps"] - 1
    st["needs_reset"][frozen] = 1
    return st, dict(frozen=frozen, parked=parked, late=late)


def prepare(c, orc):
    """reset, then the case's special lanes; returns (observations, set_state arguments or None, masks)"""
    obs = orc.reset()
    st, masks = special_state(c, orc)
    if st is not None:
        orc.set_state(**st)
        obs = observations(orc)
    return obs, st, masks


_REFERENCE = {}


def reference(learner, name, host, compute_units=None):
    """(oracle, restatement, set_state arguments, masks) after the case's run; computed once per case and left unchanged"""
    key = (learner, name, compute_units)
    if key not in _REFERENCE:
        c = case_of(name, compute_units)
        o = new_oracle(c)
        obs, st, masks = prepare(c, o)
        ref = new_restatement(learner, o.nS, host)
        ref.run(o, obs, c["T"])
        _REFERENCE[key] = (o, ref, st, masks)
    return _REFERENCE[key]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_games_host(tmp_path_factory.mktemp("games_edges"))


# ---- every case reaches what it is for ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("learner", LEARNERS)
def test_case_T_truncates_and_terminates(host, learner):
    c = CASES["T"]
    o, ref = reference(learner, "T", host)[:2]
    print("%s: %d truncated, %d terminated of %d transitions" % (learner, ref.n_truncated, ref.n_terminated, c["n"] * c["T"]))
    # (more truncated than terminated transitions: some truncated ones were not terminated, whichever way the flags overlap)
    assert ref.n_truncated > ref.n_terminated > 0 and ref.n_left_out == 0
    assert int(ref.visits.sum()) == c["n"] * c["T"] and ref.n_truncated <= int(o.hist.sum()) <= ref.n_truncated + ref.n_terminated
    if learner == "q_learning":
        assert (ref.n_truncated, ref.n_terminated) == (45132, 11855)
    if learner == "wolf_phc":
        print("ep > ea %d times, else %d times, min() clamped %d times" % (ref.n_win, ref.n_lose, ref.n_clamp))
        assert ref.n_win > 0 and ref.n_lose > 0 and ref.n_clamp > 0


@pytest.mark.parametrize("learner", LEARNERS)
def test_with_max_steps_1_every_transition_truncates_and_q_moves_by_bootstrap_alone(host, learner):
    c = CASES["T every transition truncates"]
    o, ref = reference(learner, "T every transition truncates", host)[:2]
    assert (ref.n_truncated, ref.n_terminated, ref.n_left_out) == (c["n"] * c["T"], 0, 0) == (40990, 0, 0)
    assert o.hist.tolist() == [0, c["n"] * c["T"], 0]
    s = ref.state()
    moved = [s[k] for k in ("Q", "Q_a", "Q_b") if k in s]
    assert all((q[1:] != 1.0).any() and (q[1:] > 0.0).all() for q in moved)      # no reward was seen: gamma * V alone


@pytest.mark.parametrize("name", ["S", "S uint8 end of t"])
@pytest.mark.parametrize("learner", LEARNERS)
def test_case_S_mixes_frozen_parked_late_and_plain_lanes(host, learner, name):
    c = CASES[name]
    o, ref, st, m = reference(learner, name, host)
    assert (int(m["frozen"].sum()), int(m["parked"].sum()), int(m["late"].sum())) == (820, 469, 256)
    assert not (m["frozen"] & m["parked"]).any() and not (m["late"] & (m["frozen"] | m["parked"])).any()
    # the frozen lanes every step, the parked ones on the first step alone (their episode ends there and they are reset)
    assert ref.n_left_out == 820 * c["T"] + 469
    assert ref.n_truncated >= 256 and ref.n_terminated > 0
    assert int(ref.visits.sum()) == c["n"] * c["T"] - ref.n_left_out
    assert o.misuse == 820 * c["T"]
    for k in ("row_a", "col_a", "row_b", "col_b", "t"):
        np.testing.assert_array_equal(getattr(o, k)[m["frozen"]], st[k][m["frozen"]])
    assert (st["t"][m["late"]] == c["max_steps"] - 1).all() and int(st["t"].max()) == c["max_steps"] - 1


def test_the_late_lanes_of_case_S_truncate_on_the_first_step(host):
    for name in ("S", "S uint8 end of t"):
        c = CASES[name]
        o = new_oracle(c)
        obs, st, m = prepare(c, o)
        ref = new_restatement("q_learning", o.nS, host)
        ref.run(o, obs, 1)
        assert ref.n_truncated == 256 and ref.n_left_out == 820 + 469
        assert (o.t[m["late"]] == 0).all()                         # all of them were reset, by the limit or by a goal


@pytest.mark.parametrize("learner", LEARNERS)
def test_case_W_on_one_compute_unit(host, learner):
    c = grid_wrap_case(1)
    assert c["n"] == 4096 + 259 > 8 * 256
    o, ref, st, m = reference(learner, "W", host, compute_units=1)
    assert int(m["frozen"].sum()) == 52 and m["frozen"][:c["n"] - 259].sum() == 0
    assert ref.n_left_out == 52 * c["T"] and ref.n_truncated > 0 and ref.n_terminated > 0
    assert ref.n_truncated <= int(o.hist.sum()) <= ref.n_truncated + ref.n_terminated


@pytest.mark.parametrize("learner", LEARNERS)
def test_case_L_terminates_on_the_tall_pitch(host, learner):
    o, ref = reference(learner, "L", host)[:2]
    assert o.nS == 12641 and (o.W * o.H) ** 2 * 4 == 50176 > 48 * 1024       # the observation table alone
    assert ref.n_terminated > 0 and ref.n_left_out == 0


@pytest.mark.parametrize("learner", LEARNERS)
def test_case_G_terminates_and_truncates_where_the_table_leaves_lds(host, learner):
    c = CASES["G"]
    o, ref = reference(learner, "G", host)[:2]
    table, moves = (o.W * o.H) ** 2 * 4, (2 * o.W * o.H * 5 + 16) * 4
    assert o.nS == 56113 and table == 153664 and table + moves > 150 * 1024 > moves          # soccer_create's line
    print("%s: %d truncated, %d terminated of %d transitions" % (learner, ref.n_truncated, ref.n_terminated, c["n"] * c["T"]))
    assert ref.n_truncated >= c["n"] and ref.n_terminated >= 100 and ref.n_left_out == 0
    assert int(ref.visits.sum()) == c["n"] * c["T"] and (o.hist > 0).all()


@pytest.mark.parametrize("learner", LEARNERS)
def test_case_O_depends_on_the_lane_offset(host, learner):
    o, ref = reference(learner, "O", host)[:2]
    o0, ref0 = reference(learner, "O at offset 0", host)[:2]
    assert ref.n_truncated > 0 and ref.n_terminated > 0 and ref.n_left_out == 0
    assert o.lane_offset + o.n > 2 ** 32 > o.lane_offset
    key = "Q" if learner == "minimax_q" else "Q_a"
    assert ref.state()[key].tobytes() != ref0.state()[key].tobytes() and (o.row_a != o0.row_a).any()


# ---- the restatement tells the transitions apart --------------------------------------------------------------------------------
def mutant_run(q, orc, obs, n_steps, mutant):
    """run_learner with one mistake: 'truncated counts as terminated' or 'next state taken from obs'"""
    obs = np.asarray(obs).astype(np.uint16)
    for _ in range(int(n_steps)):
        ma, mb = q.tables()
        a, b = orc.sample_actions_mixed(obs, ma, mb)
        out = orc.step(a, b)
        term = out["terminated"] | out["truncated"] if mutant == "truncated counts as terminated" else out["terminated"]
        nxt = out["obs"] if mutant == "next state taken from obs" else out["final_obs"]
        q.update(obs, a, b, out["reward"], term, nxt)
        obs = out["obs"]


@pytest.mark.parametrize("mutant", ["truncated counts as terminated", "next state taken from obs"])
@pytest.mark.parametrize("learner", LEARNERS)
def test_a_mutated_restatement_differs_in_case_T(host, learner, mutant):
    c = CASES["T"]
    ref = reference(learner, "T", host)[1]
    o = new_oracle(c)
    bad = new_restatement(learner, o.nS, host)
    mutant_run(bad, o, o.reset(), c["T"], mutant)
    key = "Q" if learner == "minimax_q" else "Q_a"
    differ = int((bad.state()[key] != ref.state()[key]).sum())
    print("%s, %s: %d of %d entries of %s differ" % (learner, mutant, differ, ref.state()[key].size, key))
    assert differ > 0
    if learner == "q_learning":
        assert ref.state()[key].size == 3805 and differ > 3700


# ---- the lane filter on a hand case -----------------------------------------------------------------------------------------------
def _hand_lanes(which):
    """an oracle whose lanes are, in this order, those of `which`: 'frozen', 'parked' (in a goal tuple, not needing reset), 'plain'"""
    c = dict(w=5, h=4, slip=0.0, n=len(which), max_steps=100)
    o = new_oracle(c)
    o.reset()
    st = dict(row_a=o.row_a.copy(), col_a=o.col_a.copy(), row_b=o.row_b.copy(), col_b=o.col_b.copy(), poss=(o.poss & 1).astype(np.uint8),
              needs_reset=np.zeros(len(which), np.uint8))
    for i, w in enumerate(which):
        if w == "parked":
            st["row_a"][i], st["col_a"][i], st["row_b"][i], st["col_b"][i], st["poss"][i] = a_goal_tuple(o)
        st["needs_reset"][i] = w == "frozen"
    o.set_state(**st)
    return o, observations(o)


TABLES = {"minimax_q": ("Q", "V", "pi_a", "pi_b", "visits"), "q_learning": ("Q_a", "Q_b", "visits"),
          "wolf_phc": ("Q_a", "Q_b", "pi_a", "pi_b", "avg_a", "avg_b", "visits", "updates")}


@pytest.mark.parametrize("learner", LEARNERS)
def test_frozen_and_parked_lanes_leave_every_table_unchanged_and_a_plain_lane_moves_its_cell(host, learner):
    o, obs = _hand_lanes(["frozen", "parked"])
    assert obs[1] == 0 and obs[0] != 0
    q = new_restatement(learner, o.nS, host, q_init=0.5)
    before = {k: np.array(q.state()[k]) for k in TABLES[learner]}
    q.run(o, obs, 1)
    s = q.state()
    for k in TABLES[learner]:
        assert np.asarray(s[k]).tobytes() == before[k].tobytes(), k
    assert (q.n_left_out, q.steps, q.alpha) == (2, 1, 0.99) and o.misuse == 1
    assert o.poss[0] & 2 and not o.poss[1] & 2 and o.hist.tolist() == [0, 1, 0]    # the parked lane's episode ended; it was reset

    o, obs = _hand_lanes(["frozen", "parked", "plain"])
    q = new_restatement(learner, o.nS, host, q_init=0.5)
    a, b = o.sample_actions_mixed(obs, *q.tables())
    s0, a0, b0 = int(obs[2]), int(a[2]), int(b[2])
    q.run(o, obs, 1)
    s = q.state()
    assert q.n_left_out == 2 and int(s["visits"].sum()) == 1 and int(s["visits"][s0, a0 * 5 + b0]) == 1
    if learner == "minimax_q":
        moved = np.argwhere(s["Q"] != before["Q"]).tolist()
        assert moved == [[s0, a0, b0]]
    else:
        assert np.argwhere(s["Q_a"] != before["Q_a"]).tolist() == [[s0, a0]]
        assert np.argwhere(s["Q_b"] != before["Q_b"]).tolist() == [[s0, b0]]
    if learner == "wolf_phc":
        assert np.flatnonzero(s["updates"]).tolist() == [s0]
        assert np.unique(np.argwhere(s["pi_a"] != before["pi_a"])[:, 0]).tolist() == [s0]
