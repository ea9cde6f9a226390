"""The settings in which tests/test_gpu_population_edges.py holds the three per-lane learner populations (Q-learners, WoLF-PHC,
minimax-Q) to their numpy restatements, defined once, and what can be said about them without a GPU: every case reaches the
path it is for (same-state, terminated, truncated-only and left-out transitions, counted by the restatements' run()), and the
comparison would catch the mistakes a kernel that carries the current state's rows in registers can make: a bootstrap from obs
where final_obs is meant, a truncated transition taken for a terminated one, an update on a goal-parked lane, a frozen member
whose alpha stands still.  This guards the yardstick where there is no GPU.  The lanes' special mixes, their preparation and
the goal tuple are those of tests/test_learner_edges_np.py."""
import os
import sys

import numpy as np
import pytest

from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from league_np import QLeagueNumpy  # noqa: E402
from minimax_q_population_np import MinimaxQPopulationNumpy, assert_minimax_q_population_equal  # noqa: E402
from om_population_np import OMPopulationNumpy  # noqa: E402
from q_learning_np import thresholds  # noqa: E402
from q_population_np import QPopulationNumpy, assert_population_equal  # noqa: E402
from wolf_population_np import WolfPopulationNumpy, assert_wolf_population_equal  # noqa: E402
from test_learner_edges_np import a_goal_tuple, prepare, special_state  # noqa: E402,F401
from test_matrix_game_host import build_games_host  # noqa: E402

GAMMA, SEED = 0.9, 1994
KINDS = ("q", "wolf", "minimax_q")
# as in the run tests of each population: greedy / greedy; learn / learn with decaying deltas; minimax-Q against itself
KW = {"q": dict(explor=0.2, decay=0.99),
      "wolf": dict(explor=0.2, decay=0.99, delta_win=0.1, delta_lose=0.4, delta_decay=0.98),
      "minimax_q": dict(explor=0.2, decay=0.99, alpha=0.8, opponent="self")}
CONFIGS = ("learn", "fixed")            # "fixed" runs in cases S and T1 alone
LDS_TABLE_LIMIT = 150 * 1024            # the observation and move tables stay in global memory beyond it

# name -> width, height, slip, members (= lanes), max_steps, steps, lane offset, how lanes are prepared after reset()
CASES = {
    "T1": dict(w=5, h=4, slip=0.0, n=259, max_steps=1, T=40),
    "S": dict(w=5, h=4, slip=0.2, n=259, max_steps=9, T=12, special="mixed"),
    "S250": dict(w=5, h=4, slip=0.2, n=259, max_steps=250, T=12, special="mixed"),
    "O": dict(w=5, h=4, slip=0.2, n=259, max_steps=6, T=20, lane_offset=2 ** 32 - 130),
    "L": dict(w=5, h=16, slip=0.2, n=67, max_steps=100, T=30),
    # 12x14 is the smallest pitch whose tables leave LDS.  Slip, members and max_steps are chosen so that every kind both
    # terminates and truncates in 30 steps (test_case_G_leaves_the_tables_in_global_memory): with 3 members, slip 0 and
    # max_steps 4 the Q kind terminated nothing.
    "G": dict(w=12, h=14, slip=0.2, n=17, max_steps=7, T=30),
    # the same pitch without slip, for the <SLIP = false, LUT_LDS = false> run kernels of the four thread-per-member populations
    # (G0_KINDS).  33 members: with 17 the Q and the opponent-modelling kinds terminated one episode in 30 steps, with 33 two
    # (test_case_G0_takes_every_branch_of_the_carry_rule_without_slip).
    "G0": dict(w=12, h=14, slip=0.0, n=33, max_steps=7, T=30),
}
CASES["O0"] = dict(CASES["O"], lane_offset=0)                  # the same handle at offset 0: what O must differ from
# W: two full grids of the run kernel and a ragged third, every fifth member of the third frozen.  A grid is 2 workgroups of
# 256 members for Q and WoLF (SOCCER_POP_GRID_BLOCKS=2), 64 waves of one member for minimax-Q (SOCCER_MQ_POP_WAVES=64).
W_GRID = {"q": 512, "wolf": 512, "minimax_q": 64}
W_TAIL = {"q": 259, "wolf": 259, "minimax_q": 19}
W_ENV = {"q": ("SOCCER_POP_GRID_BLOCKS", "2"), "wolf": ("SOCCER_POP_GRID_BLOCKS", "2"), "minimax_q": ("SOCCER_MQ_POP_WAVES", "64")}


def case_of(kind, name):
    if name == "W":
        return dict(w=5, h=4, slip=0.2, n=2 * W_GRID[kind] + W_TAIL[kind], max_steps=3, T=3, special="frozen tail", tail=W_TAIL[kind])
    return CASES[name]


def new_oracle(c):
    return Oracle(c["w"], c["h"], c["slip"], n=c["n"], seed=SEED, lane_offset=c.get("lane_offset", 0), autoreset=True,
                  max_steps=c["max_steps"])


def population_args(kind, config, n, nS):
    """the keyword arguments of the restatement and of the SoccerBatch method alike.  'fixed': Q: player A draws from one
    Dirichlet policy shared by all members; WoLF: player B is fixed per member; minimax-Q: the opponent is fixed per member."""
    kw = dict(KW[kind])
    if config == "fixed":
        rng = np.random.default_rng(11)
        if kind == "q":
            kw["act_a"] = rng.dirichlet(np.ones(5), nS)
        elif kind == "wolf":
            kw["act_b"] = rng.dirichlet(np.ones(5), (n, nS))
        else:
            kw["opponent"] = rng.dirichlet(np.ones(5), (n, nS))
    return kw


def new_restatement(kind, config, n, nS, host):
    kw = population_args(kind, config, n, nS)
    if kind == "q":
        return QPopulationNumpy(n, nS, GAMMA, **kw)
    if kind == "wolf":
        return WolfPopulationNumpy(n, nS, GAMMA, **kw)
    return MinimaxQPopulationNumpy(host, n, nS, GAMMA, **kw)


# From a fresh, constant table nearly every stage game is a saddle point, and in S and W all are: there minimax-Q starts, as its
# own run tests do, from a loaded state (MinimaxQPopulationNumpy.load: Q uniform in [-1, 1], solved), so that the solve inside the
# lane filter meets mixed games.  Every other case and kind starts from the tables creation gives.
LOADED = {("minimax_q", "S"), ("minimax_q", "W")}


def started_restatement(kind, name, config, n, nS, host):
    """the restatement in the state the case starts from; .start is what the device population's load() takes, or None"""
    ref = new_restatement(kind, config, n, nS, host)
    ref.start = None
    if (kind, name) in LOADED:
        ref.start = ref.load(np.random.default_rng(SEED + n))
        ref.codes[:] = 0
    return ref


def assert_read_equal(kind, got, want):
    """the comparison helper of that kind's own GPU suite: every table, alpha (WoLF: dscale and updates too) and steps"""
    {"q": assert_population_equal, "wolf": assert_wolf_population_equal, "minimax_q": assert_minimax_q_population_equal}[kind](got, want)


TABLES = {"q": ("Q_a", "Q_b"), "wolf": ("Q_a", "Q_b", "pi_a", "pi_b", "avg_a", "avg_b", "updates"), "minimax_q": ("Q", "V", "pi_a", "pi_b")}
PER_MEMBER = {"q": ("alpha",), "wolf": ("alpha", "dscale"), "minimax_q": ("alpha",)}


def snapshot(ref):
    return {k: np.array(v) for k, v in ref.state().items()}


def states_differ(kind, s1, s2):
    """the names of the arrays in which two state() snapshots differ"""
    return [k for k in TABLES[kind] + PER_MEMBER[kind] if np.asarray(s1[k]).tobytes() != np.asarray(s2[k]).tobytes()]


_REFERENCE = {}


def reference(kind, name, host, config="learn"):
    """(oracle, restatement, set_state arguments, masks) after the case's run; computed once per case and left unchanged"""
    key = (kind, name, config)
    if key not in _REFERENCE:
        c = case_of(kind, name)
        o = new_oracle(c)
        obs, st, masks = prepare(c, o)
        ref = started_restatement(kind, name, config, c["n"], o.nS, host)
        ref.run(o, obs, c["T"])
        _REFERENCE[key] = (o, ref, st, masks)
    return _REFERENCE[key]


# G0 is run by the four populations whose members are threads (pop_run_kernel, phc_pop_run_kernel, om_pop_run_kernel,
# pop_league_run_kernel): the two kinds above that are, and the opponent-modelling and the league populations through their own
# restatements with the Q kind's settings.  The GPU suites of those two take the case from here.
G0_KINDS = ("q", "wolf", "om", "league")
G0_LEAGUE_PLAYER = 1


def g0_league(nS):
    """three mixed league policies, every weight positive"""
    return np.random.default_rng(SEED).dirichlet(np.ones(5), (3, nS)), np.array([0.5, 0.2, 0.3])


def reference_g0(kind):
    """(oracle, restatement) after case G0's run; computed once per kind and left unchanged"""
    if kind in KINDS:
        return reference(kind, "G0", None)[:2]
    key = (kind, "G0", "learn")
    if key not in _REFERENCE:
        c = CASES["G0"]
        o = new_oracle(c)
        if kind == "om":
            ref = OMPopulationNumpy(c["n"], o.nS, GAMMA, **KW["q"])
        else:
            ref = QLeagueNumpy(c["n"], o.nS, GAMMA, G0_LEAGUE_PLAYER, *g0_league(o.nS), other="greedy", **KW["q"])
        ref.run(o, o.reset(), c["T"])
        _REFERENCE[key] = (o, ref)
    return _REFERENCE[key]


def counts(ref):
    codes = ", solver codes %s" % ref.codes.tolist() if hasattr(ref, "codes") else ""
    return "s' == s %d, terminated %d, truncated only %d, left out %d%s" % (ref.n_same, ref.n_terminated, ref.n_truncated_only, ref.n_left_out, codes)


def w_update_transitions(kind, nS):
    """one transition per member of case W for update(): obs, act_a, act_b, reward, terminated, next_obs; a reward is non-zero
    only on a terminated transition; member 0 has s' == s"""
    n = case_of(kind, "W")["n"]
    rng = np.random.default_rng(SEED)
    obs = rng.integers(1, nS, n); term = rng.random(n) < 0.3
    nxt = np.where(term, 0, rng.integers(0, nS, n))
    rew = np.where(term, rng.choice([-1, 1], n), 0)
    obs[0] = nxt[0] = 17; term[0] = False; rew[0] = 0
    return [obs, rng.integers(0, 5, n), rng.integers(0, 5, n), rew, term.astype(np.uint8), nxt]


_W_UPDATED = {}


def reference_w_then_update(kind, host):
    """(restatement, transitions): case W run again on an oracle and a restatement of its own, then one update() on every
    member, the frozen lanes' members included; computed once and left unchanged"""
    if kind not in _W_UPDATED:
        c = case_of(kind, "W")
        o = new_oracle(c)
        obs = prepare(c, o)[0]
        ref = started_restatement(kind, "W", "learn", c["n"], o.nS, host)
        ref.run(o, obs, c["T"])
        batch = w_update_transitions(kind, o.nS)
        ref.update(*batch)
        _W_UPDATED[kind] = (ref, batch)
    return _W_UPDATED[kind]


def assert_branches(kind, ref, c):
    """what the populations' own run tests ask of their references, in every case: WoLF takes every branch of the policy step;
    minimax-Q solves one game per accepted transition, none fails, and mixed games go through the simplex path"""
    if kind == "wolf":
        assert ref.n_win > 0 and ref.n_lose > 0 and ref.n_clamp > 0
    if kind == "minimax_q":
        assert ref.codes[0] > 0 and ref.codes[3] == 0 and int(ref.codes.sum()) == c["n"] * c["T"] - ref.n_left_out
    assert ref.n_same > 0 and ref.steps == c["T"]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_games_host(tmp_path_factory.mktemp("games_pop_edges"))


# ---- every case reaches what it is for ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("kind", KINDS)
def test_case_T1_every_transition_truncates_and_q_moves_by_bootstrap_alone(host, kind, config):
    c = CASES["T1"]
    o, ref = reference(kind, "T1", host, config)[:2]
    print("%s %s T1: %s" % (kind, config, counts(ref)))
    assert_branches(kind, ref, c)
    assert (ref.n_truncated_only, ref.n_terminated, ref.n_left_out) == (259 * 40, 0, 0) and c["n"] * c["T"] == 259 * 40
    assert o.hist.tolist() == [0, 10360, 0]
    s = ref.state()
    for k in ("Q", "Q_a", "Q_b"):                               # no reward was seen: gamma * V alone
        if k in s:
            assert (s[k][:, 1:] != 1.0).any() and (s[k][:, 1:] > 0.0).all(), k


@pytest.mark.parametrize("config,name", [("learn", "S"), ("fixed", "S"), ("learn", "S250")])
@pytest.mark.parametrize("kind", KINDS)
def test_case_S_mixes_frozen_parked_late_and_plain_lanes(host, kind, config, name):
    c = CASES[name]
    o, ref, st, m = reference(kind, name, host, config)
    print("%s %s %s: %s" % (kind, config, name, counts(ref)))
    assert_branches(kind, ref, c)
    assert (int(m["frozen"].sum()), int(m["parked"].sum()), int(m["late"].sum())) == (52, 30, 16)
    assert not (m["frozen"] & m["parked"]).any() and not (m["late"] & (m["frozen"] | m["parked"])).any()
    # the frozen lanes every step, the parked ones on the first step alone (their episode ends there and they are reset)
    assert ref.n_left_out == 52 * 12 + 30 == 654
    assert ref.n_truncated_only >= 16 and ref.n_terminated > 0
    assert o.misuse == 52 * c["T"]
    for k in ("row_a", "col_a", "row_b", "col_b", "t"):
        np.testing.assert_array_equal(getattr(o, k)[m["frozen"]], st[k][m["frozen"]])
    assert (st["t"][m["late"]] == c["max_steps"] - 1).all()
    if name == "S250":
        assert int(st["t"].max()) == 249


@pytest.mark.parametrize("kind", KINDS)
def test_a_parked_lane_of_case_S_draws_from_row_0_of_the_fixed_thresholds(host, kind):
    """the fixed player's row for a parked lane is row 0 of its thresholds: the shared policy's for Q, the member's own else"""
    c = CASES["S"]
    o = new_oracle(c)
    obs, st, m = prepare(c, o)
    assert (obs[m["parked"]] == 0).all() and (obs[~m["parked"] & ~m["frozen"]] != 0).all()
    ref = new_restatement(kind, "fixed", c["n"], o.nS, host)
    p = 0 if kind == "q" else 1
    rows = ref._rows(p, obs)
    pol = population_args(kind, "fixed", c["n"], o.nS)["act_a" if kind == "q" else ("act_b" if kind == "wolf" else "opponent")]
    for i in np.flatnonzero(m["parked"]):
        want = thresholds((pol[0] if kind == "q" else pol[i, 0])[None])[0]
        assert rows[i].tolist() == want.tolist()
    assert len({rows[i].tobytes() for i in np.flatnonzero(m["parked"])}) == (1 if kind == "q" else 30)


@pytest.mark.parametrize("kind", KINDS)
def test_case_O_depends_on_the_lane_offset(host, kind):
    c = CASES["O"]
    o, ref = reference(kind, "O", host)[:2]
    o0, ref0 = reference(kind, "O0", host)[:2]
    print("%s O: %s" % (kind, counts(ref)))
    assert_branches(kind, ref, c)
    assert c["lane_offset"] < 2 ** 32 < c["lane_offset"] + c["n"]
    assert ref.n_truncated_only > 0 and ref.n_terminated > 0 and ref.n_left_out == 0
    key = "Q" if kind == "minimax_q" else "Q_a"
    assert ref.state()[key].tobytes() != ref0.state()[key].tobytes() and (o.row_a != o0.row_a).any()


@pytest.mark.parametrize("kind", KINDS)
def test_case_L_terminates_on_the_tall_pitch(host, kind):
    c = CASES["L"]
    o, ref = reference(kind, "L", host)[:2]
    print("%s L: %s" % (kind, counts(ref)))
    assert_branches(kind, ref, c)
    assert o.nS == 12641 and 48 * 1024 < 2 * o.tables()[0].size <= LDS_TABLE_LIMIT
    assert ref.n_terminated > 0 and ref.n_left_out == 0


@pytest.mark.parametrize("kind", KINDS)
def test_case_G_leaves_the_tables_in_global_memory(host, kind):
    c = CASES["G"]
    o, ref = reference(kind, "G", host)[:2]
    print("%s G: %s" % (kind, counts(ref)))
    assert_branches(kind, ref, c)
    lut = o.tables()[0]
    assert o.nS == 56113 and 2 * lut.size == 153664 and 2 * lut.size > LDS_TABLE_LIMIT and c["n"] <= 33
    assert ref.n_terminated > 0 and ref.n_truncated_only > 0 and ref.n_left_out == 0
    # one pitch row less and the tables fit again: this is the smallest pitch of its width that leaves LDS
    assert 2 * ((c["w"] + 2) * (c["h"] - 1)) ** 2 * 2 <= LDS_TABLE_LIMIT and 2 * ((c["w"] + 1) * c["h"]) ** 2 * 2 <= LDS_TABLE_LIMIT


@pytest.mark.parametrize("kind", G0_KINDS)
def test_case_G0_takes_every_branch_of_the_carry_rule_without_slip(kind):
    """what the GPU cases on 12x14 at slip 0 rest on: the restatement alone shows an episode that terminates (a reload after
    the reset), one that truncates (a reload, and a bootstrap from final_obs), an update with s' == s (the registers already
    hold what was written); the league holds two picks at once"""
    c = CASES["G0"]
    o, ref = reference_g0(kind)
    print("%s G0: %s" % (kind, counts(ref)))
    assert (c["w"], c["h"], c["slip"]) == (CASES["G"]["w"], CASES["G"]["h"], 0.0) and o.nS == 56113 and c["n"] <= 33
    assert 2 * o.tables()[0].size > LDS_TABLE_LIMIT
    assert ref.n_terminated >= 1 and ref.n_truncated_only >= 1 and ref.n_same >= 1 and ref.n_left_out == 0
    assert ref.steps == c["T"]
    if kind == "wolf":
        assert_branches(kind, ref, c)
    if kind == "league":
        assert ref.max_live >= 2 and len(ref.seen - {-1}) >= 2 and ref.n_redraws > 0


@pytest.mark.parametrize("kind", KINDS)
def test_case_W_has_its_frozen_lanes_in_the_third_grid_alone(host, kind):
    c = case_of(kind, "W")
    grid, tail = W_GRID[kind], W_TAIL[kind]
    assert c["n"] == {"q": 2 * 512 + 259, "wolf": 2 * 512 + 259, "minimax_q": 2 * 64 + 19}[kind] == 2 * grid + tail
    o, ref, st, m = reference(kind, "W", host)
    print("%s W: %s" % (kind, counts(ref)))
    assert_branches(kind, ref, c)
    n_frozen = int(m["frozen"].sum())
    assert not m["frozen"][:2 * grid].any() and n_frozen == {259: 52, 19: 4}[tail]
    assert not m["parked"].any() and not m["late"].any()
    assert ref.n_left_out == n_frozen * c["T"]
    assert o.misuse == n_frozen * c["T"]
    # then one update() on every member, the frozen lanes' members included: members of all three grids move (a goal for
    # player A on a cell that still holds q_init = 1 moves nothing, so not every member does)
    ref2, batch = reference_w_then_update(kind, host)
    key = "Q" if kind == "minimax_q" else "Q_a"
    moved = (ref2.state()[key] != ref.state()[key]).reshape(c["n"], -1).any(1)
    assert moved[:grid].any() and moved[grid:2 * grid].any() and moved[2 * grid:].any() and moved[m["frozen"]].any()
    assert moved.sum() > c["n"] // 2 and ref2.steps == c["T"] + 1
    assert (batch[0] != 0).all() and (batch[0] == batch[5]).any() and batch[4].any() and not batch[4].all()


# ---- the comparison would catch the mistakes these kernels can make --------------------------------------------------------------
VARIANTS = {"bootstrap from obs": "T1", "truncated counts as terminated": "T1", "parked lanes update": "S", "frozen alpha held": "S250"}


def variant_run(q, orc, obs, n_steps, variant=None):
    """QPopulationNumpy.run (which all three restatements use) with one mistake; variant None: run() itself"""
    obs = np.asarray(obs).astype(np.uint16)
    for _ in range(int(n_steps)):
        frozen = ((orc.poss >> 1) & 1) != 0
        keep = ~frozen if variant == "parked lanes update" else ~frozen & (obs != 0)
        a, b = orc.sample_actions_mixed(q.lanes, q._rows(0, obs), q._rows(1, obs))
        out = orc.step(a, b)
        term = out["terminated"] | out["truncated"] if variant == "truncated counts as terminated" else out["terminated"]
        nxt = out["obs"] if variant == "bootstrap from obs" else out["final_obs"]
        held = {k: getattr(q, k)[frozen].copy() for k in ("alpha", "dscale") if hasattr(q, k)}
        q.update(obs, a, b, out["reward"], term, nxt, keep)
        if variant == "frozen alpha held":                     # (for WoLF dscale as well)
            for k, v in held.items():
                getattr(q, k)[frozen] = v
        obs = out["obs"]
    return obs


def _variant_state(kind, name, host, variant):
    c = CASES[name]
    o = new_oracle(c)
    obs = prepare(c, o)[0]
    q = started_restatement(kind, name, "learn", c["n"], o.nS, host)
    variant_run(q, o, obs, c["T"], variant)
    return snapshot(q)


@pytest.mark.parametrize("name", ["T1", "S"])
@pytest.mark.parametrize("kind", KINDS)
def test_the_variant_loop_without_a_mistake_is_run(host, kind, name):
    assert states_differ(kind, _variant_state(kind, name, host, None), reference(kind, name, host)[1].state()) == []


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("kind", KINDS)
def test_a_mistaken_restatement_differs_in_its_case(host, kind, variant):
    name = VARIANTS[variant]
    differ = states_differ(kind, _variant_state(kind, name, host, variant), reference(kind, name, host)[1].state())
    print("%s, %s, case %s: differs in %s" % (kind, variant, name, differ))
    if variant == "frozen alpha held":
        assert differ == list(PER_MEMBER[kind])                # alpha (WoLF: dscale too), and nothing else
    elif variant == "parked lanes update" and kind == "q":
        # The one pair that cannot differ, whatever the inputs: a step from a goal tuple stays there with reward 0, terminated,
        # final_obs 0 (oracle/soccer_oracle.c, the st == ns branch), and row 0 is zeros, so the update it would make is
        # Q[0][a] = 0 + alpha * ((0 + gamma * 0) - 0) = +0.0, the bits already there; a Q-population has no other per-state
        # array (no visits, no updates, no strategies) for it to leave a trace in.  For this kind the filter changes no result.
        assert differ == []
    else:
        assert set(differ) & set(TABLES[kind])
    if variant == "parked lanes update" and kind != "q":       # what moved is row 0 of the parked members: never a current state
        key = {"wolf": "updates", "minimax_q": "pi_a"}[kind]
        parked = reference(kind, name, host)[3]["parked"]
        got, want = _variant_state(kind, name, host, variant)[key], reference(kind, name, host)[1].state()[key]
        assert (got[parked, 0] != want[parked, 0]).reshape(30, -1).any(1).all() and (got[~parked, 0] == want[~parked, 0]).all()
