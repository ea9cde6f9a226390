"""The vectorised numpy restatement of the population of minimax-Q learners (tests/minimax_q_population_np.py) is n separate
one-lane minimax-Q learners (tests/minimax_q_np.py, member i fed lane i's transitions through update()) bit for bit, does what
the definition says on a hand case, meets the solver's simplex path in every short run the GPU tests repeat and its enumeration
fallback in the update() case, and learns: against a uniform opponent every member's table takes the reward's sign at the
cells that score, and its V moves towards the minimax values of Shapley's iteration.  tests/test_gpu_minimax_q_population.py pins the device to this restatement bit for bit, so this guards
the yardstick where there is no GPU."""
import os
import sys
import time

import numpy as np
import pytest

from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from minimax_q_np import MinimaxQNumpy, shapley_lists, shapley_vi  # noqa: E402
from minimax_q_population_np import MinimaxQPopulationNumpy, assert_minimax_q_population_equal  # noqa: E402
from test_matrix_game_host import build_games_host  # noqa: E402

GAMMA = 0.9


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_games_host(tmp_path_factory.mktemp("games_mqpop"))


# ---- the short runs tests/test_gpu_minimax_q_population.py repeats on the device ---------------------------------------------
T_RUN, SEED = 60, 1994
RUN_KW = dict(explor=0.2, decay=0.99, alpha=0.8)
# width, height, slip, opponent, members, max_steps.  Member counts: a single wave, more members than one CU holds waves, an odd
# count.  Every case starts from a loaded state (MinimaxQPopulationNumpy.load: Q uniform in [-1, 1], solved): a fresh table is
# constant, so every early stage game would be a saddle point.
RUN_CASES = [(5, 4, 0.0, "uniform", 1, 100),
             (5, 4, 0.2, "self", 67, 5),
             (5, 4, 0.2, "dirichlet", 259, 5),
             (5, 4, 0.0, "uniform", 259, 100),
             (7, 5, 0.0, "self", 67, 100),
             (7, 5, 0.2, "fixed", 67, 5),
             (11, 7, 0.2, "uniform", 3, 100)]
RUN_IDS = ["5x4 slip 0 uniform 1", "5x4 slip 0.2 self truncating 67", "5x4 slip 0.2 fixed per member truncating 259", "5x4 slip 0 uniform 259",
           "7x5 slip 0 self 67", "7x5 slip 0.2 fixed shared truncating 67", "11x7 slip 0.2 uniform 3"]


def opponent_of(name, n, nS):
    """'dirichlet': a fixed policy per member; 'fixed': one for every member"""
    if isinstance(name, str) and name == "dirichlet":
        return np.random.default_rng(11).dirichlet(np.ones(5), (n, nS))
    if isinstance(name, str) and name == "fixed":
        return np.random.default_rng(12).dirichlet(np.ones(5), nS)
    return name


_REFERENCE = {}


def reference_run(L, w, h, slip, opponent, n, max_steps=100, T=T_RUN, seed=SEED):
    """(oracle, restatement, the loaded state it started from) after T steps; computed once per case and left unchanged"""
    key = (w, h, slip, opponent, n, max_steps, T, seed)
    if key not in _REFERENCE:
        o = Oracle(w, h, slip, n=n, seed=seed, autoreset=True, max_steps=max_steps)
        ref = MinimaxQPopulationNumpy(L, n, o.nS, GAMMA, opponent=opponent_of(opponent, n, o.nS), **RUN_KW)
        start = ref.load(np.random.default_rng(seed + n))
        ref.codes[:] = 0
        ref.run(o, o.reset(), T)
        _REFERENCE[key] = (o, ref, start)
    return _REFERENCE[key]


@pytest.mark.parametrize("case", RUN_CASES, ids=RUN_IDS)
def test_the_short_runs_solve_mixed_games(host, case):
    w, h, slip, opponent, n, max_steps = case
    o, ref, start = reference_run(host, w, h, slip, opponent, n, max_steps)
    print("%dx%d slip %g, opponent %s, %d members, max_steps %d: solver codes simplex %d, saddle point %d, enumeration %d, none passed %d; "
          "s' == s %d, terminated %d, truncated only %d" % ((w, h, slip, opponent, n, max_steps) + tuple(ref.codes.tolist())
                                                           + (ref.n_same, ref.n_terminated, ref.n_truncated_only)))
    assert ref.codes[0] > 0 and ref.codes[3] == 0 and int(ref.codes.sum()) == n * T_RUN
    assert ref.n_left_out == 0 and ref.steps == T_RUN
    if n > 1:
        assert ref.n_same > 0
    if max_steps == 5:
        assert ref.n_truncated_only > 0
    s = ref.state()
    assert (np.abs(s["Q"]) <= 1.0).all() and (np.abs(s["V"]) <= 1.0).all() and (s["Q"][:, 0] == 0).all() and (s["V"][:, 0] == 0).all()
    for k in ("pi_a", "pi_b"):
        assert (s[k] >= 0.0).all() and np.abs(s[k].sum(2) - 1.0).max() < 1e-12
    assert s["Q"].tobytes() != start["Q"].tobytes()


# ---- the update() case of the GPU file ---------------------------------------------------------------------------------------
UPDATE_KW = dict(decay=0.9, explor=0.2, q_init=0.5)
N_UPDATE, HARD_FIRST = 67, 30           # members HARD_FIRST.. carry a near-tie game at state 100 + i and a tiny alpha


def near_ties(rng, k):
    """the first hard family of DESIGN section 9 (tests/test_matrix_game_host.py: hard_games), halved so that it fits [-1, 1]:
    small integer games perturbed by 1e-15 .. 1e-11"""
    base = rng.integers(-1, 2, (k, 5, 5)).astype(np.float64)
    return 0.5 * (base + rng.choice([1e-15, 1e-13, 1e-11], (k, 1, 1)) * rng.integers(-1, 2, (k, 5, 5)))


def valid_transitions(rng, nS, n):
    """obs, act_a, act_b, reward, terminated, next_obs; a reward is non-zero only on a terminated transition"""
    obs = rng.integers(1, nS, n); term = rng.random(n) < 0.3
    nxt = np.where(term, 0, rng.integers(0, nS, n))
    rew = np.where(term, rng.choice([-1, 1], n), 0)
    return [obs, rng.integers(0, 5, n), rng.integers(0, 5, n), rew, term.astype(np.uint8), nxt]


def update_case(L, nS=761):
    """(restatement in its loaded state, creation parameters, what load() takes, [(transitions, keep, misuse bits)] * 3, the
    members with a bad action, those with a bad observation)"""
    n = N_UPDATE
    rng = np.random.default_rng(1994)
    alpha = np.full(n, 0.75); alpha[HARD_FIRST:] = 2.0 ** -44        # the hard members' cell moves by ~1e-14: the game stays a near-tie
    kw = dict(UPDATE_KW, alpha=alpha)
    ref = MinimaxQPopulationNumpy(L, n, nS, GAMMA, **kw)
    ref.Q[:, 1:] = rng.uniform(-1.0, 1.0, (n, nS - 1, 5, 5))
    hard = np.arange(HARD_FIRST, n)
    ref.Q[hard, 100 + hard] = near_ties(rng, hard.size)
    ref.solve()
    ref.codes[:] = 0
    start = {"Q": ref.Q.copy()}
    warm = valid_transitions(rng, nS, n)
    case = valid_transitions(rng, nS, n)

    def put(i, s, a, bb, r, term, s2):
        for k, v in enumerate((s, a, bb, r, term, s2)):
            case[k][i] = v
    put(0, 17, 2, 0, 0, 0, 17)          # s' == s: the bootstrap is V[s] before the re-solve
    put(1, 5, 0, 4, 1, 1, 0)            # terminated, next_obs 0, r = +1
    put(2, 5, 4, 4, -1, 1, 0)           # r = -1
    put(4, 17, 1, 1, 1, 1, 300)         # terminated with a live next_obs: still no bootstrap
    for i in hard:                      # the hard members' transitions hit their near-tie state, half of them with s' == s
        put(i, 100 + i, int(rng.integers(0, 5)), int(rng.integers(0, 5)), 0, 0, 100 + i if i % 2 else int(rng.integers(1, nS)))
    bad_act, bad_obs = [10, 11, 12], [20, 21, 22]
    case[1][10] = 5; case[2][11] = -1; case[1][12] = 100
    case[0][20] = 0; case[0][21] = nS; case[5][22] = nS + 3
    keep = np.ones(n, bool); keep[bad_act + bad_obs] = False
    return ref, kw, start, [(warm, None, 0), (case, keep, 2 | 4), (warm, None, 0)], bad_act, bad_obs


def test_the_update_case_meets_the_enumeration_fallback(host):
    ref, kw, start, batches, bad_act, bad_obs = update_case(host)
    for batch, keep, _ in batches:
        before = {k: v.copy() for k, v in ref.state().items() if k != "steps"}
        ref.update(*batch, keep=keep)
        if keep is not None:
            for i in bad_act + bad_obs:             # left alone, alpha advanced
                assert all(ref.state()[k][i].tobytes() == before[k][i].tobytes() for k in ("Q", "V", "pi_a", "pi_b"))
                assert ref.alpha[i] == before["alpha"][i] * 0.9
    print("update() on %d members, three batches: solver codes simplex %d, saddle point %d, enumeration %d, none passed %d" % ((N_UPDATE,) + tuple(ref.codes.tolist())))
    assert ref.codes[0] > 0 and ref.codes[2] >= 1 and ref.codes[3] == 0
    assert int(ref.codes.sum()) == 3 * N_UPDATE - len(bad_act + bad_obs) and ref.steps == 3


# ---- the vectorised restatement is n separate learners ----------------------------------------------------------------------
@pytest.mark.parametrize("opponent", ["uniform", "self", "fixed", "dirichlet"], ids=["uniform", "self", "fixed shared", "fixed per member"])
def test_the_vectorised_restatement_is_n_separate_learners_bit_for_bit(host, opponent):
    """5x4, slip 0.2, 33 members, 200 steps, max_steps = 5 so that episodes truncate; per-member arrays for all four
    hyperparameters"""
    n, T = 33, 200
    rng = np.random.default_rng(5)
    hyper = dict(alpha=rng.uniform(0.3, 1.0, n), decay=rng.uniform(0.95, 1.0, n), explor=rng.uniform(0.05, 0.6, n))
    gam = rng.uniform(0.5, 0.95, n)
    o = Oracle(5, 4, 0.2, n=n, seed=1994, autoreset=True, max_steps=5)
    opp = opponent_of(opponent, n, o.nS)
    one = lambda i: opp if isinstance(opp, str) or opp.ndim == 2 else opp[i]  # noqa: E731
    pop = MinimaxQPopulationNumpy(host, n, o.nS, gam, q_init=0.3, opponent=opp, **hyper)
    solo = [MinimaxQNumpy(host, o.nS, gam[i], q_init=0.3, opponent=one(i), **{k: v[i] for k, v in hyper.items()}) for i in range(n)]
    obs = o.reset()
    for _ in range(T):
        tabs = [q.tables() for q in solo]
        rows = [np.stack([t[0][s] for t, s in zip(tabs, obs)]), None if tabs[0][1] is None else np.stack([t[1][s] for t, s in zip(tabs, obs)])]
        for p in (0, 1):
            np.testing.assert_array_equal(rows[p], pop._rows(p, obs))       # the rows the population draws from are the members' own
        a, b = o.sample_actions_mixed(np.arange(n), rows[0], rows[1])
        out = o.step(a, b)
        for i, q in enumerate(solo):        # every lane is live here (reset above, obs never 0 on an auto-reset handle)
            q.update(obs[i:i + 1], a[i:i + 1], b[i:i + 1], out["reward"][i:i + 1], out["terminated"][i:i + 1], out["final_obs"][i:i + 1])
        same = out["final_obs"] == obs; term = out["terminated"] != 0
        pop.n_same += int(same.sum()); pop.n_terminated += int(term.sum()); pop.n_truncated_only += int((~term & (out["truncated"] != 0)).sum())
        pop.update(obs, a, b, out["reward"], out["terminated"], out["final_obs"])
        obs = out["obs"]
        assert (obs != 0).all()
    assert pop.n_same > 0 and pop.n_terminated > 0 and pop.n_truncated_only > 0, (pop.n_same, pop.n_terminated, pop.n_truncated_only)
    want = {"Q": np.stack([q.Q for q in solo]), "V": np.stack([q.V for q in solo]), "pi_a": np.stack([q.pi_a for q in solo]),
            "pi_b": np.stack([q.pi_b for q in solo]), "alpha": np.array([q.alpha for q in solo]), "steps": solo[0].steps}
    assert_minimax_q_population_equal(pop.state(), want)
    assert pop.steps == T and int(pop.codes.sum()) == n * T and (pop.pi_a != 0.2).sum() > n
    # run() is the same loop: a second population driven by run() on a second oracle ends in the same bits
    o2 = Oracle(5, 4, 0.2, n=n, seed=1994, autoreset=True, max_steps=5)
    pop2 = MinimaxQPopulationNumpy(host, n, o2.nS, gam, q_init=0.3, opponent=opp, **hyper)
    pop2.run(o2, o2.reset(), T)
    assert_minimax_q_population_equal(pop2.state(), pop.state())
    assert (pop2.n_same, pop2.n_terminated, pop2.n_truncated_only, pop2.n_left_out) == (pop.n_same, pop.n_terminated, pop.n_truncated_only, 0)
    assert pop2.codes.tolist() == pop.codes.tolist()


def test_one_member_two_steps_by_hand(host):
    """Member 1 of three, state 2 loaded with constant rows Q[a][b] = a / 8: a saddle point at (4, 0), V = 0.5.  Step 1 (alpha
    1): cell (4, 0), terminated with r = -1, becomes -1; row 4's minimum falls, the saddle point moves to (3, 0), V = 0.375.  Step 2
    (alpha 0.5) has s' == s on cell (3, 0): the target bootstraps from V = 0.375, the value BEFORE step 2's re-solve, on the 2^-40
    grid; afterwards row 3's minimum is that cell and V is the cell.  Member 0 is left out of step 2, member 2 is never kept."""
    q = MinimaxQPopulationNumpy(host, 3, 4, 0.5, alpha=1.0, decay=0.5, explor=0.2, q_init=0.0, opponent="uniform")
    row = np.repeat(np.array([0.0, 0.125, 0.25, 0.375, 0.5])[:, None], 5, 1)
    q.Q[:, 2] = row
    q.solve()
    assert q.V[:, 2].tolist() == [0.5] * 3 and q.pi_a[1, 2].tolist() == [0, 0, 0, 0, 1] and q.pi_b[1, 2].tolist() == [1, 0, 0, 0, 0]
    one = dict(obs=[2, 2, 3], act_a=[4, 4, 0], act_b=[0, 0, 0], reward=[-1, -1, 0], terminated=[1, 1, 0], next_obs=[0, 0, 1])
    q.update(keep=[True, True, False], **one)
    assert q.Q[1, 2, 4].tolist() == [-1.0, 0.5, 0.5, 0.5, 0.5] and q.V[1, 2] == 0.375
    assert q.pi_a[1, 2].tolist() == [0, 0, 0, 1, 0] and q.pi_b[1, 2].tolist() == [1, 0, 0, 0, 0]
    assert q.alpha.tolist() == [0.5] * 3 and q.steps == 1
    first = {k: v[0].copy() for k, v in q.state().items() if k not in ("steps", "alpha")}
    two = dict(obs=[2, 2, 3], act_a=[3, 3, 0], act_b=[0, 0, 0], reward=[0, 0, 0], terminated=[0, 0, 0], next_obs=[2, 2, 1])
    q.update(keep=[False, True, False], **two)
    m = 0.0 + 0.5 * (float(np.rint(0.375 * 2.0 ** 40)) * 2.0 ** -40)
    cell = 0.375 + 0.5 * (m - 0.375)
    assert cell == 0.28125 and q.Q[1, 2, 3].tolist() == [cell, 0.375, 0.375, 0.375, 0.375]
    assert q.V[1, 2] == cell and q.pi_a[1, 2].tolist() == [0, 0, 0, 1, 0] and q.pi_b[1, 2].tolist() == [1, 0, 0, 0, 0]
    assert q.alpha.tolist() == [0.25] * 3 and q.steps == 2 and q.codes.tolist() == [0, 3, 0, 0]
    # nothing else moved: the member left out, the member never kept, the other states
    assert all(q.state()[k][0].tobytes() == first[k].tobytes() for k in first)
    assert (q.Q[2, 2] == row).all() and q.V[2, 2] == 0.5 and (q.Q[:, [1, 3]] == 0.0).all() and (q.pi_a[:, 0] == 0.2).all() and (q.pi_a[:, [1, 3]] == np.eye(5)[0]).all()      # (solve() solved the zero games of states 1 and 3)


# ---- learning ------------------------------------------------------------------------------------------------------------
# the learning run of tests/test_gpu_minimax_q_population.py: Littman's MR, a learner per lane, alpha 1 -> 0.01
LEARN = dict(width=5, height=4, slip=0.0, gamma=0.9, n=64, T=100000, seed=1994, explor=0.2, q_init=0.0, alpha=1.0)
# T = 100 000.  A step of this restatement is interpreter overhead (about thirty numpy and ctypes calls) and costs 0.09 to 0.33 ms
# on the machines it has run on; T is sized for the slowest of them (33 s), so that this file stays under a minute there.
# One stream of experience from Q = 0 learns slowly: a state's strategies are first solved from a table of zeros, which gives
# the pure strategy "stand", so player A moves only by exploration; alpha falls from 1 to 0.01 over the run, so a cell's few
# visits carry a mean weight of about 0.2; and V[s] is a maximin, which stays 0 until a whole row of Q[s] is positive or every
# row has a negative entry.  Population mean (over the 64 members; min .. max member in brackets), measured with this restatement
# (learning_run below), of
#   scoring cells   the share of the scoring cells (s, a, b) — those whose expected immediate reward is at least 0.5 in size: the
#                   joint move scores unless a player slips; 760 of the 19 000 cells at either slip — where Q_i does not yet have
#                   the sign of that reward: what a learner finds out first, who scores where
#   decided states  the mean of |V_i - V*| over the states with |V*| >= 0.95 (76 at slip 0, 24 at slip 0.2), V* from shapley_vi
#   all states      the same over the 760 live states
#   seed, slip     scoring cells                       decided states                      all states
#   1994, 0        0.339844  (0.305263 .. 0.378947)    0.873911  (0.839917 .. 0.904637)    0.445925  (0.441961 .. 0.449337)
#   1,    0        0.341036  (0.318421 .. 0.373684)    0.875756  (0.849936 .. 0.901160)    0.446135  (0.443250 .. 0.449031)
#   2,    0.2      0.395539  (0.356579 .. 0.430263)    0.920701  (0.887639 .. 0.940293)    0.399267  (0.395439 .. 0.402322)
#   7,    0.2      0.399322  (0.360526 .. 0.426316)    0.919459  (0.889966 .. 0.939183)    0.399256  (0.396813 .. 0.402505)
#   untrained      1.000000                            1.000000 / 0.955973                 0.459155 at slip 0, 0.408422 at 0.2
# Twice the worst figure of either V column does NOT lie below its untrained figure (it takes 400 000 steps for the decided
# states, 0.483, and more than 500 000 for all states), so at this budget those grades would not show learning; as section 15 did,
# the grade that does is what is asserted: the scoring cells.  BOUND is twice the worst of the four (section 12's rule: the
# margin covers seed-to-seed spread, which the four runs show), 0.798644, below the untrained 1.0.  Both V figures are printed,
# and that the all-states figure improves is asserted.
BOUND = 2 * 0.399322


DECIDED = 0.95
SCORING = 0.5


def learning_grade(Q, V, lists, vstar):
    """(per-member share of the scoring cells where Q_i lacks the reward's sign — untrained: 1.0 —, per-member mean of
    |V_i - V*| over the decided states and its untrained figure (V = 0), the same two over all live states).  lists:
    minimax_q_np.shapley_lists."""
    Pp, Pn, Pr, Pd = lists
    R = (Pp * Pr).sum(2)                                               # [nS, 25] a cell's expected immediate reward
    cells = np.abs(R) >= SCORING; cells[0] = False
    Q = np.asarray(Q).reshape(len(Q), -1, 25)
    share = (np.sign(Q[:, cells]) != np.sign(R[cells])).mean(1)
    m = np.abs(vstar) >= DECIDED; m[0] = False
    return share, np.abs(V - vstar)[:, m].mean(1), np.abs(vstar[m]).mean(), np.abs(V - vstar)[:, 1:].mean(1), np.abs(vstar)[1:].mean()


def learning_run(L, seed, slip, T=LEARN["T"], n=LEARN["n"]):
    """(the population after T steps, learning_grade of it)"""
    c = LEARN
    o = Oracle(c["width"], c["height"], slip, n=n, seed=seed, autoreset=True)
    lists = shapley_lists(Oracle(c["width"], c["height"], slip, n=4, seed=seed, autoreset=True))
    vstar, _ = shapley_vi(L, lists, c["gamma"])
    q = MinimaxQPopulationNumpy(L, n, o.nS, c["gamma"], alpha=c["alpha"], decay=0.01 ** (1.0 / T), explor=c["explor"], q_init=c["q_init"],
                                opponent="uniform")
    q.run(o, o.reset(), T)
    return (q,) + learning_grade(q.Q, q.V, lists, vstar)


def test_the_restatement_learns_the_minimax_values(host):
    c = LEARN
    t0 = time.perf_counter()
    q, share, err, untrained, err_all, untrained_all = learning_run(host, c["seed"], c["slip"])
    print("MR, %d members x %d steps, seed %d: population mean of the share of scoring cells without the reward's sign %.6f (members %.6f .. "
          "%.6f), untrained 1.0; mean |V - V*| over the decided states %.6f (%.6f .. %.6f), untrained %.6f; over all live states %.6f (%.6f .. "
          "%.6f), untrained %.6f; solver codes %s; %.1f s"
          % (c["n"], c["T"], c["seed"], share.mean(), share.min(), share.max(), err.mean(), err.min(), err.max(), untrained, err_all.mean(),
             err_all.min(), err_all.max(), untrained_all, q.codes.tolist(), time.perf_counter() - t0))
    assert q.steps == c["T"] and np.abs(q.alpha - 0.01).max() < 1e-9
    assert q.n_left_out == 0 and q.n_same > 0 and q.n_terminated > 0 and q.codes[0] > 0 and q.codes[3] == 0
    assert BOUND < 1.0                          # the bound shows learning: untrained, no scoring cell has a sign
    assert share.mean() <= BOUND
    assert err_all.mean() < untrained_all and err.mean() < untrained
