"""The settings in which tests/test_gpu_population_edges.py holds the three per-lane learner populations (Q-learners, WoLF-PHC,
minimax-Q) to their numpy restatements, defined once, and what can be said about them without a GPU: every case reaches the
path it is for (same-state, terminated, truncated-only and left-out transitions, counted by the restatements' run()), and the
comparison would catch the mistakes a kernel that carries the current state's rows in registers can make: a bootstrap from obs
where final_obs is meant, a truncated transition taken for a terminated one, an update on a goal-parked lane, a frozen member
whose alpha stands still.  This guards the yardstick where there is no GPU.  The lanes' special mixes, their preparation and
the goal tuple are those of tests/test_learner_edges_np.py.

Three more kinds run the same cases with the Q kind's settings: the opponent-modelling population (om_pop_run_kernel, which
carries the pair (g_A[s], g_B[s]) instead of rows) and the Q population against a league that plays A or B
(pop_league_run_kernel, which carries a pick beside the rows).  They add the mistakes those two kernels alone can make, and
case H: a league run that ends exactly at tick 2^62, where the host refuses to go on, and one whose tick's low word carries;
and case D: crafted rows at the edges of the opponent-modelling population's derived values (no count, a tie, a skewed count,
counts beyond 2^53), an update() that bootstraps from them and a greedy step that acts on them."""
import os
import sys

import numpy as np
import pytest

from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from league_np import QLeagueNumpy, assert_league_equal, league_pick  # noqa: E402
from minimax_q_population_np import MinimaxQPopulationNumpy, assert_minimax_q_population_equal  # noqa: E402
from om_population_np import OMPopulationNumpy, assert_om_population_equal, derive  # noqa: E402
from philox_np import lane_words  # noqa: E402
from q_learning_np import observations, thresholds  # noqa: E402
from q_population_np import QPopulationNumpy, assert_population_equal  # noqa: E402
from wolf_population_np import WolfPopulationNumpy, assert_wolf_population_equal  # noqa: E402
from test_learner_edges_np import a_goal_tuple, prepare, special_state  # noqa: E402,F401
from test_matrix_game_host import build_games_host  # noqa: E402

GAMMA, SEED = 0.9, 1994
KINDS = ("q", "wolf", "minimax_q")
# the opponent-modelling population, and the Q population whose player A / player B is a league: the settings of KW["q"]
NEW_KINDS = ("om", "league_a", "league_b")
ALL_KINDS = KINDS + NEW_KINDS
LEAGUE_PLAYER = {"league_a": 0, "league_b": 1}
# as in the run tests of each population: greedy / greedy; learn / learn with decaying deltas; minimax-Q against itself
KW = {"q": dict(explor=0.2, decay=0.99),
      "wolf": dict(explor=0.2, decay=0.99, delta_win=0.1, delta_lose=0.4, delta_decay=0.98),
      "minimax_q": dict(explor=0.2, decay=0.99, alpha=0.8, opponent="self")}
for _k in NEW_KINDS:
    KW[_k] = KW["q"]
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
# H, for the league as player B alone: the tick is set after the reset so that the run ends exactly at 2^62 (the league's draw
# is the Philox block at counter 2^62 + tick, and the host refuses a run that would cross tick 2^62), or so that the tick's
# low word carries during the run; at slip 0 and at slip 0.2
CASES["H"] = dict(w=5, h=4, slip=0.2, n=67, max_steps=5, T=20)
H_SLIPS = (0.0, 0.2)
H_TICKS = (2 ** 62 - 20, 2 ** 32 - 7)
# W: two full grids of the run kernel and a ragged third, every fifth member of the third frozen.  A grid is 2 workgroups of
# 256 members for Q and WoLF (SOCCER_POP_GRID_BLOCKS=2), 64 waves of one member for minimax-Q (SOCCER_MQ_POP_WAVES=64).
W_GRID = {"q": 512, "wolf": 512, "minimax_q": 64}
W_TAIL = {"q": 259, "wolf": 259, "minimax_q": 19}
W_ENV = {"q": ("SOCCER_POP_GRID_BLOCKS", "2"), "wolf": ("SOCCER_POP_GRID_BLOCKS", "2"), "minimax_q": ("SOCCER_MQ_POP_WAVES", "64")}
for _k in NEW_KINDS:                                            # members are threads, as for Q and WoLF
    W_GRID[_k], W_TAIL[_k], W_ENV[_k] = W_GRID["q"], W_TAIL["q"], W_ENV["q"]


def case_of(kind, name):
    if name == "W":
        return dict(w=5, h=4, slip=0.2, n=2 * W_GRID[kind] + W_TAIL[kind], max_steps=3, T=3, special="frozen tail", tail=W_TAIL[kind])
    return CASES[name]


def new_oracle(c):
    return Oracle(c["w"], c["h"], c["slip"], n=c["n"], seed=SEED, lane_offset=c.get("lane_offset", 0), autoreset=True,
                  max_steps=c["max_steps"])


def population_args(kind, config, n, nS):
    """the keyword arguments of the restatement and of the SoccerBatch method alike.  'fixed': Q: player A draws from one
    Dirichlet policy shared by all members; WoLF: player B is fixed per member; minimax-Q: the opponent is fixed per member;
    the opponent-modelling kind: as Q.  The league kinds: the league of g0_league plays its player, the other player is greedy
    or, 'fixed', draws from that same Dirichlet policy; the arguments are the SoccerBatch method's (new_restatement translates)."""
    kw = dict(KW[kind])
    if kind in LEAGUE_PLAYER:
        other = np.random.default_rng(11).dirichlet(np.ones(5), nS) if config == "fixed" else "greedy"
        acts = ("league", other) if LEAGUE_PLAYER[kind] == 0 else (other, "league")
        pol, w = g0_league(nS)
        kw.update(act_a=acts[0], act_b=acts[1], league_policies=pol, league_weights=w)
        return kw
    if config == "fixed":
        rng = np.random.default_rng(11)
        if kind in ("q", "om"):
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
    if kind == "om":
        return OMPopulationNumpy(n, nS, GAMMA, **kw)
    if kind in LEAGUE_PLAYER:
        p = LEAGUE_PLAYER[kind]
        acts = (kw.pop("act_a"), kw.pop("act_b"))
        assert acts[p] == "league"
        return QLeagueNumpy(n, nS, GAMMA, p, kw.pop("league_policies"), kw.pop("league_weights"), other=acts[1 - p], **kw)
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
    {"q": assert_population_equal, "wolf": assert_wolf_population_equal, "minimax_q": assert_minimax_q_population_equal,
     "om": assert_om_population_equal, "league_a": assert_league_equal, "league_b": assert_league_equal}[kind](got, want)


# (a league's read() is its tables with picks() under "pick", as QLeagueNumpy.state() has them)
TABLES = {"q": ("Q_a", "Q_b"), "wolf": ("Q_a", "Q_b", "pi_a", "pi_b", "avg_a", "avg_b", "updates"), "minimax_q": ("Q", "V", "pi_a", "pi_b"),
          "om": ("Q_a", "Q_b", "C_a", "C_b"), "league_a": ("Q_a", "Q_b", "pick"), "league_b": ("Q_a", "Q_b", "pick")}
PER_MEMBER = {"q": ("alpha",), "wolf": ("alpha", "dscale"), "minimax_q": ("alpha",), "om": ("alpha",), "league_a": ("alpha",),
              "league_b": ("alpha",)}


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
    if kind in LEAGUE_PLAYER:                                   # different picks live at once, and a lane draws more than once
        assert ref.max_live >= 2 and ref.n_redraws > 0 and len(ref.seen - {-1}) >= 2
    if kind == "om":                                            # updates at states with no count yet (n = 0) and with counts
        assert 0 < ref.n_first_seen < c["n"] * c["T"] - ref.n_left_out
    assert ref.n_same > 0 and ref.steps == c["T"]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_games_host(tmp_path_factory.mktemp("games_pop_edges"))


# ---- every case reaches what it is for ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("kind", ALL_KINDS)
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
    if kind in NEW_KINDS and config == "learn":                 # how often the reset landed on s again
        assert ref.n_same == {"om": 1051, "league_a": 355, "league_b": 335}[kind]
    if kind in LEAGUE_PLAYER:
        # every lane draws at every step, all but the first time again; after the last step every pick is cleared
        assert ref.n_redraws == 259 * 39 == 10101 and ref.max_live == 3 and ref.seen == {0, 1, 2} and (ref.pick == -1).all()


@pytest.mark.parametrize("config,name", [("learn", "S"), ("fixed", "S"), ("learn", "S250")])
@pytest.mark.parametrize("kind", ALL_KINDS)
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
    if kind in LEAGUE_PLAYER:                                   # a frozen lane keeps the pick of its one draw
        assert set(ref.pick[m["frozen"]].tolist()) == {0, 1, 2}
    if kind == "om":                                            # a parked lane left no count in row 0
        assert not ref.C_a[:, 0].any() and not ref.C_b[:, 0].any()


@pytest.mark.parametrize("kind", sorted(LEAGUE_PLAYER))
def test_frozen_and_parked_lanes_of_case_S_draw_a_pick_at_kick_off(kind):
    """the league's draw sits before the lane filter: at the first step every lane draws, the frozen lanes keep what they drew
    for good, the parked lanes finish their episode there and draw again at the second step"""
    c = CASES["S"]
    o = new_oracle(c)
    obs, st, m = prepare(c, o)
    ref = new_restatement(kind, "learn", c["n"], o.nS, None)
    tick0 = o.tick
    obs = ref.run(o, obs, 1)
    first = league_pick(ref.T, lane_words(SEED, np.arange(c["n"]), 2 ** 62 + tick0, purpose=1))
    assert ref._drawn.all() and ref.n_redraws == 0
    assert (ref.pick[m["frozen"]] == first[m["frozen"]]).all() and (ref.pick[m["parked"]] == -1).all()
    assert len(set(first[m["parked"]].tolist())) == 3
    ref.run(o, obs, 1)
    assert ref.n_redraws >= 30 and (ref.pick[m["frozen"]] == first[m["frozen"]]).all()


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


@pytest.mark.parametrize("kind", ALL_KINDS)
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


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_case_L_terminates_on_the_tall_pitch(host, kind):
    c = CASES["L"]
    o, ref = reference(kind, "L", host)[:2]
    print("%s L: %s" % (kind, counts(ref)))
    assert_branches(kind, ref, c)
    assert o.nS == 12641 and 48 * 1024 < 2 * o.tables()[0].size <= LDS_TABLE_LIMIT
    assert ref.n_terminated > 0 and ref.n_left_out == 0
    if kind in NEW_KINDS:
        assert ref.n_terminated == {"om": 8, "league_a": 19, "league_b": 21}[kind]
    if kind in LEAGUE_PLAYER:
        assert ref.max_live == 3


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


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_case_W_has_its_frozen_lanes_in_the_third_grid_alone(host, kind):
    c = case_of(kind, "W")
    grid, tail = W_GRID[kind], W_TAIL[kind]
    assert c["n"] == {"minimax_q": 2 * 64 + 19}.get(kind, 2 * 512 + 259) == 2 * grid + tail
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
    if kind in NEW_KINDS:
        assert ref.n_left_out == 52 * 3 == 156 and ref.n_terminated > 0
    if kind in LEAGUE_PLAYER:                                   # update() is no step of a lane: every pick stays
        assert ref2.pick.tolist() == ref.pick.tolist() and (ref.pick >= 0).any() and (ref.pick == -1).any()


# ---- the comparison would catch the mistakes these kernels can make --------------------------------------------------------------
VARIANTS = {"bootstrap from obs": "T1", "truncated counts as terminated": "T1", "parked lanes update": "S", "frozen alpha held": "S250"}


# the mistakes pop_league_run_kernel alone can make with the pick it carries beside the rows, and the case each shows in
LEAGUE_VARIANTS = {"frozen pick cleared": "S", "frozen pick redrawn": "S", "no draw off the field": "S",
                   "redraw after terminated only": "T1", "draw without the lane offset": "O"}


def variant_run(q, orc, obs, n_steps, variant=None):
    """QPopulationNumpy.run (which the restatements use; QLeagueNumpy.run for a league, with the draw before the step and the
    clearing after it) with one mistake; variant None: run() itself"""
    obs = np.asarray(obs).astype(np.uint16)
    league = isinstance(q, QLeagueNumpy)
    for _ in range(int(n_steps)):
        frozen = ((orc.poss >> 1) & 1) != 0
        keep = ~frozen if variant == "parked lanes update" else ~frozen & (obs != 0)
        if league:
            need = q.pick < 0
            if variant == "frozen pick redrawn":
                need = need | frozen
            if variant == "no draw off the field":              # the draw moved behind the lane filter: these lanes keep -1, which
                need = need & ~frozen & (obs != 0)              # as an index is the last policy; their step takes no action anyway
            ids = q.lanes if variant == "draw without the lane offset" else orc.lane_offset + q.lanes
            W = lane_words(orc.seed, ids, 2 ** 62 + orc.tick, purpose=1)
            q.pick = np.where(need, league_pick(q.T, W), q.pick).astype(np.int32)
        a, b = orc.sample_actions_mixed(q.lanes, q._rows(0, obs), q._rows(1, obs))
        out = orc.step(a, b)
        term = out["terminated"] | out["truncated"] if variant == "truncated counts as terminated" else out["terminated"]
        nxt = out["obs"] if variant == "bootstrap from obs" else out["final_obs"]
        held = {k: getattr(q, k)[frozen].copy() for k in ("alpha", "dscale") if hasattr(q, k)}
        q.update(obs, a, b, out["reward"], term, nxt, keep)
        if variant == "frozen alpha held":                     # (for WoLF dscale as well)
            for k, v in held.items():
                getattr(q, k)[frozen] = v
        if league:
            ended = (out["terminated"] != 0) if variant == "redraw after terminated only" else (out["terminated"] != 0) | (out["truncated"] != 0)
            finished = ~frozen & ended
            if variant == "frozen pick cleared":
                finished = finished | frozen
            q.pick = np.where(finished, -1, q.pick).astype(np.int32)
        obs = out["obs"]
    return obs


def om_carried_run(q, orc, obs, n_steps, mistake=None):
    """OMPopulationNumpy.run for (greedy, greedy) restated the way om_pop_run_kernel acts: not from the rows at s but from the
    pair (g_A[s], g_B[s]) it carries over the steps — the pair derived at s' BEFORE the update while the episode goes on, the
    pair the update left at s when the lane stays at s, the pair derived anew after a reset.  mistake None: the kernel's rule,
    whose result is run()'s; 'pair of final_obs carried over a reset': the pair of s' = final_obs taken for the next step
    although the lane was reset to another state."""
    assert q.act == ("greedy", "greedy")
    s = np.asarray(obs).astype(np.int64)
    g = [q._derive(p, q.lanes, s)[1] for p in (0, 1)]
    e = q.explor[:, None]
    for _ in range(int(n_steps)):
        keep = (((orc.poss >> 1) & 1) == 0) & (s != 0)
        rows = [thresholds((1.0 - e) * np.eye(5)[g[p]] + e / 5.0) for p in (0, 1)]
        a, b = orc.sample_actions_mixed(q.lanes, rows[0], rows[1])
        out = orc.step(a, b)
        s2, sn = out["final_obs"].astype(np.int64), out["obs"].astype(np.int64)
        before = [q._derive(p, q.lanes, s2)[1] for p in (0, 1)]
        q.update(s, a, b, out["reward"], out["terminated"], s2, keep)
        goes_on = keep if mistake == "pair of final_obs carried over a reset" else keep & (sn == s2)
        assert mistake in (None, "pair of final_obs carried over a reset")
        for p in (0, 1):
            at_s, at_sn = q._derive(p, q.lanes, s)[1], q._derive(p, q.lanes, sn)[1]      # after the update
            g[p] = np.where(sn == s, at_s, np.where(goes_on, before[p], at_sn))
        s = sn
    return s.astype(np.uint16)


def _variant_state(kind, name, host, variant):
    c = CASES[name]
    o = new_oracle(c)
    obs = prepare(c, o)[0]
    q = started_restatement(kind, name, "learn", c["n"], o.nS, host)
    variant_run(q, o, obs, c["T"], variant)
    return snapshot(q)


@pytest.mark.parametrize("name", ["T1", "S"])
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_the_variant_loop_without_a_mistake_is_run(host, kind, name):
    assert states_differ(kind, _variant_state(kind, name, host, None), reference(kind, name, host)[1].state()) == []


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_a_mistaken_restatement_differs_in_its_case(host, kind, variant):
    name = VARIANTS[variant]
    differ = states_differ(kind, _variant_state(kind, name, host, variant), reference(kind, name, host)[1].state())
    print("%s, %s, case %s: differs in %s" % (kind, variant, name, differ))
    if variant == "frozen alpha held":
        assert differ == list(PER_MEMBER[kind])                # alpha (WoLF: dscale too), and nothing else
    elif variant == "parked lanes update" and kind in ("q", "league_a", "league_b"):
        # The one pair that cannot differ, whatever the inputs: a step from a goal tuple stays there with reward 0, terminated,
        # final_obs 0 (oracle/soccer_oracle.c, the st == ns branch), and row 0 is zeros, so the update it would make is
        # Q[0][a] = 0 + alpha * ((0 + gamma * 0) - 0) = +0.0, the bits already there; a Q-population has no other per-state
        # array (no visits, no updates, no strategies) for it to leave a trace in.  For this kind the filter changes no result.
        # A league adds the picks alone, and a parked lane's pick is drawn before the filter and cleared after its step
        # whether it updates or not: the same holds for the two league kinds.
        assert differ == []
    else:
        assert set(differ) & set(TABLES[kind])
    if variant == "parked lanes update" and kind == "om":      # row 0 of the parked members' counts: one count per player
        parked = reference(kind, name, host)[3]["parked"]
        got = _variant_state(kind, name, host, variant)
        assert differ == ["C_a", "C_b"]
        for k in differ:
            assert (got[k][parked, 0].sum(1) == 1).all() and not got[k][~parked, 0].any()
    if variant == "parked lanes update" and kind in ("wolf", "minimax_q"):       # what moved is row 0 of the parked members: never a current state
        key = {"wolf": "updates", "minimax_q": "pi_a"}[kind]
        parked = reference(kind, name, host)[3]["parked"]
        got, want = _variant_state(kind, name, host, variant)[key], reference(kind, name, host)[1].state()[key]
        assert (got[parked, 0] != want[parked, 0]).reshape(30, -1).any(1).all() and (got[~parked, 0] == want[~parked, 0]).all()


@pytest.mark.parametrize("variant", sorted(LEAGUE_VARIANTS))
@pytest.mark.parametrize("kind", sorted(LEAGUE_PLAYER))
def test_a_mistake_with_the_carried_pick_differs_in_its_case(kind, variant):
    name = LEAGUE_VARIANTS[variant]
    got, (o, ref, st, m) = _variant_state(kind, name, None, variant), reference(kind, name, None)
    differ = states_differ(kind, got, ref.state())
    print("%s, %s, case %s: differs in %s" % (kind, variant, name, differ))
    assert "pick" in differ
    if name == "S":
        # a frozen lane's pick steers nothing (its lane does not move), so the picks of the frozen lanes are where these show, and
        # the only place: every other lane, the parked ones from their second step on, draws and plays as in run()
        f = m["frozen"]
        assert differ == ["pick"] and (got["pick"][~f] == ref.pick[~f]).all() and (got["pick"][f] != ref.pick[f]).any()
        if variant != "frozen pick redrawn":                    # (redrawn at the last step: a value, but of another tick)
            assert (got["pick"][f] == -1).all()
    else:
        assert set(differ) >= {"Q_a", "Q_b", "pick"}            # other policies were played: the tables moved otherwise
    if variant == "redraw after terminated only":              # nothing terminates in T1: every lane still holds its first pick
        first = league_pick(ref.T, lane_words(SEED, np.arange(CASES[name]["n"]), 2 ** 62 + 1, purpose=1))       # (reset() took tick 0)
        assert got["pick"].tolist() == first.tolist() and (ref.pick == -1).all()


@pytest.mark.parametrize("name", ["T1", "S"])
def test_the_carried_pair_without_a_mistake_is_run(name):
    """the rule by which om_pop_run_kernel carries (g_A[s], g_B[s]), restated on the restatement's tables, gives what run()
    gives from the rows: where every step resets (T1), and with frozen, parked and late lanes (S)"""
    c = CASES[name]
    o = new_oracle(c)
    obs = prepare(c, o)[0]
    q = new_restatement("om", "learn", c["n"], o.nS, None)
    om_carried_run(q, o, obs, c["T"])
    o0, ref = reference("om", name, None)[:2]
    assert states_differ("om", snapshot(q), ref.state()) == []
    assert o.row_a.tolist() == o0.row_a.tolist() and o.hist.tolist() == o0.hist.tolist()


def test_a_pair_carried_over_a_reset_differs_in_case_T1():
    c = CASES["T1"]
    o = new_oracle(c)
    q = new_restatement("om", "learn", c["n"], o.nS, None)
    om_carried_run(q, o, prepare(c, o)[0], c["T"], "pair of final_obs carried over a reset")
    o0, ref = reference("om", "T1", None)[:2]
    differ = states_differ("om", snapshot(q), ref.state())
    print("om, pair of final_obs carried over a reset, case T1: differs in %s" % differ)
    # (the lanes themselves cannot tell: with max_steps = 1 every lane ends on its last reset, whatever was played)
    assert differ == ["Q_a", "Q_b", "C_a", "C_b"]


# ---- H: the league's counter 2^62 + tick at the end of its range, and a tick whose low word carries -----------------------------
_H = {}


def reference_h(slip, tick):
    """(oracle, restatement) of case H after its run, the oracle's tick set to `tick` after the reset (None: left at 1);
    computed once and left unchanged"""
    if (slip, tick) not in _H:
        c = dict(CASES["H"], slip=slip)
        o = new_oracle(c)
        obs = o.reset()
        if tick is not None:
            o.tick = tick
        ref = new_restatement("league_b", "learn", c["n"], o.nS, None)
        ref.run(o, obs, c["T"])
        _H[(slip, tick)] = (o, ref)
    return _H[(slip, tick)]


@pytest.mark.parametrize("tick", H_TICKS, ids=["2^62-20", "2^32-7"])
@pytest.mark.parametrize("slip", H_SLIPS)
def test_case_H_terminates_truncates_and_redraws_at_a_high_tick(slip, tick):
    c = CASES["H"]
    o, ref = reference_h(slip, tick)
    print("league_b H slip %s from tick %d: %s, %d redraws, picks seen %s" % (slip, tick, counts(ref), ref.n_redraws, sorted(ref.seen)))
    assert o.tick == tick + c["T"] and ref.steps == c["T"] and ref.n_left_out == 0
    if tick == 2 ** 62 - 20:
        assert o.tick == 2 ** 62                                # one step more and the draw's counter would leave its range
        assert (ref.n_terminated, ref.n_truncated_only, ref.n_redraws) == {0.0: (16, 252, 213), 0.2: (25, 244, 218)}[slip]
    else:
        assert tick < 2 ** 32 < o.tick
    assert ref.n_terminated > 0 and ref.n_truncated_only > 100 and ref.n_redraws > 100 and ref.seen == {0, 1, 2} and ref.max_live == 3
    o1, ref1 = reference_h(slip, None)                          # the same run at tick 1
    assert o1.tick == 1 + c["T"]
    assert states_differ("league_b", snapshot(ref), ref1.state())[:2] == ["Q_a", "Q_b"] and (o.row_a != o1.row_a).any()


# ---- D: the derived values (V, g) of the opponent-modelling population at the edges of their definition -----------------------------
# read() derives V and pi in numpy, so what the DEVICE derives (om_derive: after load() in a kernel of its own, after an update
# inside it) shows only in what is done with it: the cell an update moves (V at next_obs) and the action a greedy step takes (g at
# the lane's state).  Case D loads crafted rows at six live states of 5x4, a kind of row per (member, state, player), then makes
# one update() per member and one run(1) with explor = 0.
D_ROWS = ("n = 0", "tie", "skewed", "clamp +", "clamp -", "plain")
D_BIG = 2 ** 53 + 3                     # as a float64 it rounds to 2^53 + 4 (tests/test_om_population_np.py)
D_N = 24
D_KW = dict(KW["q"], explor=0.0)


def d_row(name, rng):
    """(Q [5, 5], C [5] as Python ints) of one crafted row"""
    Q = rng.uniform(-1.0, 1.0, (5, 5))
    if name == "n = 0":                 # nothing seen beside a non-constant Q: the row means
        return Q, [0] * 5
    if name == "tie":                   # actions 1, 3 and 4 attain the maximum: the first index wins
        return np.array([[0.25] * 5, [0.5] * 5, [-1.0] * 5, [0.5] * 5, [0.5] * 5]), [2, 0, 7, 0, 1]
    if name == "skewed":                # only columns 0 and 4 weigh
        return Q, [3, 0, 0, 0, 1]
    if name == "clamp +":               # W[g] / N = (2^53 + 6) / (2^53 + 4) > 1
        return np.array([[1.0] * 5] + [[0.5] * 5] * 4), [D_BIG, 2, 0, 0, 0]
    if name == "clamp -":
        return np.full((5, 5), -1.0), [D_BIG, 2, 0, 0, 0]
    return Q, [int(x) for x in rng.integers(1, 9, 5)]


def d_kind(i, k, p):
    """which row member i holds at state k for player p: over six consecutive members a state shows every kind to both players"""
    return (i + k + 3 * p) % 6


_D = {}


def derive_case():
    """case D, computed once and left unchanged: 'c' the handle's settings, 'S' the six states, 'start' what load() takes,
    'batch' the update's transitions, 'place' the set_state arguments of the run, 'k_next' / 'k_obs' / 'k_run' the index into S of
    every member's next_obs, obs and lane; and the restatement: 'loaded', 'updated', 'ran' = state() snapshots, 'oracle' after
    the run, 'acts' = the pair of actions every member must take in the run, by derive() on the rows it stood on"""
    if _D:
        return _D
    n = D_N
    c = dict(w=5, h=4, slip=0.2, n=n, max_steps=100)
    scratch = new_oracle(dict(c, n=64))                        # six different live states: where lanes stand after three steps
    scratch.reset()
    for _ in range(3):
        scratch.step(*scratch.sample_actions())
    obs = observations(scratch)
    live = (obs != 0) & (((scratch.poss >> 1) & 1) == 0)
    lanes = [int(np.flatnonzero(live & (obs == s))[0]) for s in np.unique(obs[live])[:6]]
    S = obs[lanes].astype(np.int64)
    assert len(set(S.tolist())) == 6
    ref = OMPopulationNumpy(n, scratch.nS, GAMMA, **D_KW)
    rng = np.random.default_rng(SEED)
    for i in range(n):
        for k in range(6):
            for p, (Q, C) in enumerate(((ref.Q_a, ref.C_a), (ref.Q_b, ref.C_b))):
                Q[i, S[k]], row = d_row(D_ROWS[d_kind(i, k, p)], rng)
                C[i, S[k]] = np.array(row, np.uint64)
    loaded = snapshot(ref)
    # the update: next_obs is a crafted state (V as the load derived it), obs another one (the update derives it again)
    k_next = (np.arange(n) // 6 % 2) * 3
    k_obs = (k_next + 1) % 6
    batch = [S[k_obs], rng.integers(0, 5, n), rng.integers(0, 5, n), np.zeros(n, np.int64), np.zeros(n, np.uint8), S[k_next]]
    ref.update(*batch)
    updated = snapshot(ref)
    # the run: the first twelve lanes stand on the row the update derived again, the others on a row only the load derived
    k_run = np.where(np.arange(n) < 12, k_obs, (k_next + 2) % 6)
    src = np.array(lanes)[k_run]
    place = dict(row_a=scratch.row_a[src], col_a=scratch.col_a[src], row_b=scratch.row_b[src], col_b=scratch.col_b[src],
                 poss=(scratch.poss[src] & 1).astype(np.uint8), t=np.zeros(n, scratch.t.dtype), needs_reset=np.zeros(n, np.uint8))
    o = new_oracle(c)
    o.reset()
    o.set_state(**place)
    assert observations(o).tolist() == S[k_run].tolist()
    acts = [ref._derive(p, ref.lanes, S[k_run])[1] for p in (0, 1)]
    ref.run(o, observations(o), 1)
    _D.update(c=c, S=S, start={k: loaded[k] for k in ("Q_a", "Q_b", "C_a", "C_b")}, batch=batch, place=place, k_next=k_next, k_obs=k_obs,
              k_run=k_run, loaded=loaded, updated=updated, ran=snapshot(ref), oracle=o, acts=acts, ref=ref)
    return _D


def test_case_D_holds_every_edge_of_the_derived_values_for_both_players():
    d = derive_case()
    S, n = d["S"], D_N
    for p, (Q, C) in enumerate((("Q_a", "C_a"), ("Q_b", "C_b"))):
        V, g = derive(d["loaded"][Q][:, S], d["loaded"][C][:, S])                              # [n, 6]
        kinds = np.array([[d_kind(i, k, p) for k in range(6)] for i in range(n)])
        name = lambda x: kinds == D_ROWS.index(x)  # noqa: E731
        assert (V[name("tie")] == 0.5).all() and (g[name("tie")] == 1).all()
        assert (V[name("clamp +")] == 1.0).all() and (V[name("clamp -")] == -1.0).all() and (g[name("clamp +")] == 0).all()
        rows = d["loaded"][Q][:, S][name("n = 0")]
        means = ((((rows[..., 0] + rows[..., 1]) + rows[..., 2]) + rows[..., 3]) + rows[..., 4]) / 5.0
        assert (V[name("n = 0")] == means.max(1)).all() and (g[name("n = 0")] == means.argmax(1)).all()
        rows = d["loaded"][Q][:, S][name("skewed")]
        W = 3.0 * rows[..., 0] + 1.0 * rows[..., 4]
        assert (V[name("skewed")] == W.max(1) / 4.0).all() and len(set(g[name("skewed")].tolist())) > 1
        # what the update bootstraps from, and what the run acts on: every kind of row, for this player
        assert {d_kind(i, d["k_next"][i], p) for i in range(n)} == set(range(6))
        assert {d_kind(i, d["k_run"][i], p) for i in range(12)} == {d_kind(i, d["k_run"][i], p) for i in range(12, n)} == set(range(6))
        assert len(set(d["acts"][p].tolist())) >= 4
    # the update moved one cell per player and member in a crafted row, and raised one count there: exact beyond 2^53
    assert (d["k_obs"] != d["k_next"]).all() and (d["k_run"][:12] == d["k_obs"][:12]).all()
    assert (d["k_run"][12:] != d["k_obs"][12:]).all() and (d["k_run"][12:] != d["k_next"][12:]).all()
    up, ld = d["updated"], d["loaded"]
    assert ((up["Q_a"] != ld["Q_a"]).sum((1, 2, 3)) == 1).all() and ((up["C_a"] - ld["C_a"]).sum((1, 2)) == 1).all()
    big = [int(x) for x in up["C_a"][up["C_a"] > 2 ** 53]]
    assert D_BIG in big and D_BIG + 1 in big                    # an odd count that no float64 holds, and one that was raised
    # the run: every member took the pair derive() names, on its crafted row
    ran = d["ran"]
    for p, C, other in ((0, "C_a", 1), (1, "C_b", 0)):
        rose = (ran[C] - up[C])[np.arange(n), S[d["k_run"]]]
        assert (rose.sum(1) == 1).all() and (rose.argmax(1) == d["acts"][other]).all()
