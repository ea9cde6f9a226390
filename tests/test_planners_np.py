"""tests/planners_np.py pinned where there is no GPU: the list family bit for bit to the oracle's Python loops and to the
reference's fixtures (5x4, both learners; the loops also on 7x5), the sparse rows bit for bit to the oracle's dense
Pmat / Rmat, the dense family to the oracle's numpy-dot versions and the fixtures within the project's rounding bound for
them (numpy's BLAS dot associates differently from a sequential sum) with identical counters and greedy policies, and the
sweep cap."""
import glob
import os
import sys

import numpy as np
import pytest

from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planners_np as pn  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
VI = sorted(glob.glob(os.path.join(GOLD, "vi_*.npz")))
PL = sorted(glob.glob(os.path.join(GOLD, "planners_*.npz")))
DENSE_RTOL, DENSE_ATOL = 1e-12, 1e-14                          # tests/test_planner.py's bound for the dense planners

_games = {}


def _ids(paths):
    return [os.path.basename(p)[:-4] for p in paths]


def game(w, h, slip, learner, policy):
    """(oracle, P, lists, rows), built once per game"""
    key = (w, h, slip, learner, np.asarray(policy).tobytes())
    if key not in _games:
        orc = O.Oracle(w, h, slip)
        P = O.single_agent_lists(orc, learner, policy)
        lists = pn.pad_lists(P, orc.nS)
        rows = pn.sparse_rows(P, orc.nS, int(np.count_nonzero(orc.tables()[1] == 2)), lists)
        _games[key] = (orc, P, lists, rows)
    return _games[key]


def fixture(path):
    d = np.load(path)
    return d, game(5, 4, float(d["slip"]), bytes(d["learner"]).decode(), d["policy"]), float(d["theta"]), float(d["discount_factor"])


def same_bits(got, want, what):
    g = np.ascontiguousarray(got); w = np.ascontiguousarray(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if g.dtype == np.float64:
        g = g.view(np.int64); w = np.ascontiguousarray(w, np.float64).view(np.int64)
    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    assert bad.size == 0, "%s differs in %d entries, first at flat index %d: %r vs %r" % (
        what, bad.size, bad[0], np.asarray(got).reshape(-1)[bad[0]], np.asarray(want).reshape(-1)[bad[0]])


def random_game(w, h, slip, learner, seed):
    orc = O.Oracle(w, h, slip)
    return game(w, h, slip, learner, np.random.default_rng(seed).integers(0, 5, orc.nS).astype(np.int8))


def test_fixtures_cover_both_learners():
    learners = {bytes(np.load(p)["learner"]).decode() for p in VI + PL}
    assert learners == {"player_a", "player_b"} and len(PL) >= 2


# ---- the list family ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", VI, ids=_ids(VI))
def test_value_iteration_is_the_fixture_and_the_oracle_loop(path):
    d, (orc, P, lists, _), theta, gamma = fixture(path)
    r = pn.value_iteration(lists, theta, gamma)
    assert r.counter == int(d["iterations"]) and not r.capped
    same_bits(r.V, d["V"], "V"); same_bits(r.Q, d["Q"], "Q"); same_bits(r.pi, d["pi"], "pi")
    pi, V, Q, cc = O.value_iteration(P, orc.nS, 1e-3, 0.8)
    r = pn.value_iteration(lists, 1e-3, 0.8)
    assert r.counter == cc
    same_bits(r.V, V, "V"); same_bits(r.Q, Q, "Q"); same_bits(r.pi, pi, "pi")
    # the cap: the oracle's loop stops the same way (`or cc >= max_iterations`)
    pi, V, Q, cc = O.value_iteration(P, orc.nS, 1e-3, 0.8, max_iterations=5)
    r = pn.value_iteration(lists, 1e-3, 0.8, max_sweeps=5)
    assert r.capped and r.counter == cc == 5
    same_bits(r.V, V, "capped V"); same_bits(r.Q, Q, "capped Q"); same_bits(r.pi, pi, "capped pi")


@pytest.mark.parametrize("path", PL, ids=_ids(PL))
def test_list_planners_are_the_fixtures(path):
    d, (orc, P, lists, _), theta, gamma = fixture(path)
    r = pn.policy_evaluation(lists, d["pe_pi"], theta, gamma)
    same_bits(r.V, d["pe_V"], "pe_V")
    imp = pn.policy_improvement(lists, r.V, gamma)
    same_bits(imp.pi, d["imp_pi"], "imp_pi"); same_bits(imp.Q, d["imp_Q"], "imp_Q")
    r = pn.policy_iteration(lists, d["pi_pi0"], theta, gamma)
    assert r.counter == int(d["pi_iterations"]) and not r.capped
    same_bits(r.pi, d["pi_pi"], "pi_pi"); same_bits(r.V, d["pi_V"], "pi_V"); same_bits(r.Q, d["pi_Q"], "pi_Q")


@pytest.mark.parametrize("path", PL, ids=_ids(PL))
def test_list_planners_are_the_oracle_loops_5x4(path):
    d, (orc, P, lists, _), _, _ = fixture(path)
    V, sweeps = O.policy_evaluation(d["pe_pi"], P, orc.nS, 1e-4, 0.9)
    r = pn.policy_evaluation(lists, d["pe_pi"], 1e-4, 0.9)
    assert r.counter == sweeps
    same_bits(r.V, V, "V")
    pi, Q = O.policy_improvement(V, P, orc.nS, 0.9)
    imp = pn.policy_improvement(lists, V, 0.9)
    same_bits(imp.pi, pi, "pi"); same_bits(imp.Q, Q, "Q")
    pi, V, Q, cc = O.policy_iteration(P, orc.nS, d["pi_pi0"], 1e-4, 0.9)
    r = pn.policy_iteration(lists, d["pi_pi0"], 1e-4, 0.9)
    assert r.counter == cc and cc >= 2
    same_bits(r.pi, pi, "pi"); same_bits(r.V, V, "V"); same_bits(r.Q, Q, "Q")


def test_list_planners_are_the_oracle_loops_7x5():
    orc, P, lists, _ = random_game(7, 5, 0.3, "player_b", 5)
    rng = np.random.default_rng(6)
    pi, V, Q, cc = O.value_iteration(P, orc.nS, 1e-8, 0.9)
    r = pn.value_iteration(lists, 1e-8, 0.9)
    assert r.counter == cc and cc > 50
    same_bits(r.V, V, "V"); same_bits(r.Q, Q, "Q"); same_bits(r.pi, pi, "pi")
    pe = rng.integers(0, 5, orc.nS)
    V, sweeps = O.policy_evaluation(pe, P, orc.nS, 1e-3, 0.8)
    r = pn.policy_evaluation(lists, pe, 1e-3, 0.8)
    assert r.counter == sweeps
    same_bits(r.V, V, "pe V")
    Vin = rng.uniform(-1, 1, orc.nS)
    pi, Q = O.policy_improvement(Vin, P, orc.nS, 0.9)
    imp = pn.policy_improvement(lists, Vin, 0.9)
    same_bits(imp.pi, pi, "imp pi"); same_bits(imp.Q, Q, "imp Q")
    pi, V, Q, cc = O.policy_iteration(P, orc.nS, pe, 1e-8, 0.7)
    r = pn.policy_iteration(lists, pe, 1e-8, 0.7)
    assert r.counter == cc and cc >= 2
    same_bits(r.pi, pi, "pi pi"); same_bits(r.V, V, "pi V"); same_bits(r.Q, Q, "pi Q")


# ---- the sparse rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,slip,learner", [(5, 4, 0.2, "player_a"), (5, 4, 0.2, "player_b"), (5, 4, 1.0, "player_a"),
                                              (5, 4, 0.0, "player_b"), (7, 5, 0.3, "player_b")])
def test_sparse_rows_densified_are_the_oracle_mats(w, h, slip, learner):
    orc, P, lists, rows = random_game(w, h, slip, learner, 5)
    Pmat, Rmat = O.single_agent_mats(orc, learner, np.random.default_rng(5).integers(0, 5, orc.nS))
    Mp, Mn, Rm = rows
    dense, _ = pn.densify(rows)
    same_bits(dense, Pmat, "Pmat"); same_bits(Rm, Rmat, "Rmat")
    # kept entries: non-zero, ascending next states, padding only behind them
    live = Mp != 0.0
    assert np.all(live[..., :-1] | ~live[..., 1:])
    assert np.all((np.diff(Mn, axis=-1) > 0) | ~live[..., 1:])
    assert np.count_nonzero(live) == np.count_nonzero(Pmat)
    assert Pmat[0, 0, 0] > 1.0                                  # index 0 collects every goal tuple


# ---- the dense family ---------------------------------------------------------------------------------------------------
def close(got, want):
    np.testing.assert_allclose(got, want, rtol=DENSE_RTOL, atol=DENSE_ATOL)


@pytest.mark.parametrize("path", PL, ids=_ids(PL))
def test_dense_planners_are_the_fixtures_to_rounding(path):
    d, (orc, P, lists, rows), theta, gamma = fixture(path)
    r = pn.policy_eval_dense(rows, d["de_policy"], theta, gamma, k=25, init=d["de_init"])
    assert r.counter == int(d["de_cc"]) and not r.capped
    close(r.V, d["de_v"])
    r = pn.policy_eval_dense(rows, d["de_policy"], 1e-6, 0.9)
    assert r.counter == int(d["de0_cc"])
    close(r.V, d["de0_v"])
    for tag, k, th, g in (("mpi1", 1, theta, gamma), ("mpi2", 10000000, theta, gamma), ("mpi3", 5, 1e-6, 0.9)):
        r = pn.modified_policy_iteration(rows, k, th, g)
        assert r.counter == int(d[tag + "_counter"]) and not r.capped, tag
        same_bits(r.pi, d[tag + "_pi"], tag + " pi")
        close(r.V, d[tag + "_V"]); close(r.Q, d[tag + "_Q"])


@pytest.mark.parametrize("w,h,slip,learner", [(5, 4, 0.2, "player_a"), (5, 4, 1.0, "player_b"), (7, 5, 0.3, "player_b")])
def test_dense_planners_are_the_oracle_numpy_versions_to_rounding(w, h, slip, learner):
    orc, P, lists, rows = random_game(w, h, slip, learner, 5)
    Pmat, Rmat = pn.densify(rows)                               # the oracle's, bit for bit (above)
    rng = np.random.default_rng(7)
    pol = rng.dirichlet(np.ones(5), orc.nS); init = rng.uniform(-1, 1, orc.nS)
    v, cc = O.policy_eval_dense(Pmat, Rmat, pol, 1e-8, 0.9, k=7, init=init.copy())
    r = pn.policy_eval_dense(rows, pol, 1e-8, 0.9, k=7, init=init)
    assert r.counter == cc == 7
    close(r.V, v)
    pi, V, Q, counter = O.modified_policy_iteration(Pmat, Rmat, 5, 1e-6, 0.9)
    r = pn.modified_policy_iteration(rows, 5, 1e-6, 0.9)
    assert r.counter == counter
    same_bits(r.pi, pi, "pi")
    close(r.V, V); close(r.Q, Q)


# ---- the cap ------------------------------------------------------------------------------------------------------------
def test_the_cap_counts_sweeps_across_evaluations():
    orc, P, lists, rows = random_game(5, 4, 0.2, "player_a", 5)
    rng = np.random.default_rng(8)
    pi0 = rng.integers(0, 5, orc.nS)
    full = pn.policy_iteration(lists, pi0, 1e-8, 0.9)
    assert not full.capped and full.sweeps > full.counter >= 2
    r = pn.policy_iteration(lists, pi0, 1e-8, 0.9, max_sweeps=full.sweeps)
    assert not r.capped and r.counter == full.counter           # the cap is reached only by a sweep that does not converge
    same_bits(r.V, full.V, "V")
    r = pn.policy_iteration(lists, pi0, 1e-8, 0.9, max_sweeps=full.sweeps - 1)
    assert r.capped and r.sweeps == full.sweeps - 1 and r.counter == full.counter
    # cut inside the first evaluation: V is that evaluation's iterate, pi one improvement from it
    r = pn.policy_iteration(lists, pi0, 1e-8, 0.9, max_sweeps=3)
    e = pn.policy_evaluation(lists, pi0, 1e-8, 0.9, max_sweeps=3)
    assert r.capped and e.capped and r.counter == 1 and r.sweeps == e.sweeps == 3
    same_bits(r.V, e.V, "V"); same_bits(r.Q, pn.policy_improvement(lists, e.V, 0.9).Q, "Q")
    # modified policy iteration: capped at a greedy step (k = 2: sweeps 1 and 4 are greedy steps) and inside an evaluation
    full = pn.modified_policy_iteration(rows, 2, 1e-8, 0.9)
    assert not full.capped and full.sweeps > 2 * full.counter
    g = pn.modified_policy_iteration(rows, 2, 1e-8, 0.9, max_sweeps=4)
    assert g.capped and g.sweeps == 4 and g.counter == 1
    same_bits(g.V, g.Q.max(1), "V = max Q at a greedy step")
    e = pn.modified_policy_iteration(rows, 2, 1e-8, 0.9, max_sweeps=5)
    assert e.capped and e.sweeps == 5 and e.counter == 2
    same_bits(e.Q, g.Q, "Q of the greedy step"); same_bits(e.pi, g.pi, "pi of the greedy step")
    one = pn.policy_eval_dense(rows, np.eye(5)[g.pi], 1e-8, 0.9, k=1, init=g.V)
    same_bits(e.V, one.V, "V one evaluation sweep from the greedy step's")
    # dense evaluation: the k-th sweep at the cap counts as capped, below it does not
    pol = rng.dirichlet(np.ones(5), orc.nS)
    assert pn.policy_eval_dense(rows, pol, 1e-8, 0.9, k=7, max_sweeps=7).capped
    r = pn.policy_eval_dense(rows, pol, 1e-8, 0.9, k=7, max_sweeps=8)
    assert not r.capped and r.counter == 7
