"""The numpy restatement of the regret matchers of one table (tests/regret_matching_np.py) does what the definition says on a
hand case and against a scalar loop, keeps its regrets where `plus` puts them, takes every branch in the short runs the GPU
tests use, and learns: in self-play the average pair is less exploitable than the uniform pair (the CPU best-response iteration
of tests/best_response_np.py).  tests/test_gpu_regret_matching.py pins the device to this restatement bit for bit, so this
guards the yardstick where there is no GPU."""
import os
import sys

import numpy as np
import pytest

from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_response_np as br  # noqa: E402
from minimax_q_np import shapley_lists  # noqa: E402
from q_learning_np import SCALE  # noqa: E402
from regret_matching_np import RegretMatchingNumpy, average, policy  # noqa: E402

GAMMA = 0.9

# ---- the short runs tests/test_gpu_regret_matching.py repeats on the device ----------------------------------------------
N_RUN, T_RUN, SEED = 8192 + 3, 60, 1994
RUN_KW = dict(explor=0.2, decay=0.99, q_init=1.0)
# width, height, slip, act_a, act_b, plus, linear, max_steps
RUN_CASES = [(5, 4, 0.0, "learn", "uniform", True, False, 100),
             (5, 4, 0.2, "learn", "learn", False, True, 100),
             (7, 5, 0.3, "dirichlet", "learn", True, True, 100),
             (11, 7, 0.2, "uniform", "learn", False, False, 100),
             (5, 4, 0.2, "learn", "learn", True, False, 5)]
RUN_IDS = ["5x4 slip 0 learn-uniform plus", "5x4 slip 0.2 learn-learn plain linear", "7x5 slip 0.3 fixed-learn plus linear",
           "11x7 slip 0.2 uniform-learn plain", "5x4 slip 0.2 max_steps 5"]


def act(name, nS):
    if isinstance(name, str) and name == "dirichlet":
        return np.random.default_rng(11).dirichlet(np.ones(5), nS)
    return name


_REFERENCE = {}


def reference_run(w, h, slip, act_a, act_b, plus, linear, max_steps=100, T=T_RUN, n=N_RUN):
    """(oracle, restatement) after T steps; computed once per case and left unchanged"""
    key = (w, h, slip, act_a, act_b, plus, linear, max_steps, T, n)
    if key not in _REFERENCE:
        o = Oracle(w, h, slip, n=n, seed=SEED, autoreset=True, max_steps=max_steps)
        ref = RegretMatchingNumpy(o.nS, GAMMA, act_a=act(act_a, o.nS), act_b=act(act_b, o.nS), plus=plus, linear=linear, **RUN_KW)
        ref.run(o, o.reset(), T)
        _REFERENCE[key] = (o, ref)
    return _REFERENCE[key]


def test_two_updates_by_hand():
    """One state, alpha = 1, the Q rows (0, 1, 0, 0, 0) and (-1, 0, 0, 0, 0) after the first update; A learns, B is uniform.
    First update: R was 0, so the policy is the 0.2 fallback, u = 0.2; action 1 regrets 0.8, the others -0.2, floored under
    plus.  Second: the policy is all on action 1, u = 1, action 1 regrets nothing more, the others -1.  Third: a transition
    into that state bootstraps with the value of each player's own policy, on the grid: A's 1.0, the uniform B's -0.2."""
    one = dict(obs=[2], act_a=[1], act_b=[0], reward=[1], terminated=[1], next_obs=[0])
    for plus, linear in ((True, False), (True, True), (False, False)):
        q = RegretMatchingNumpy(4, 0.5, alpha=1.0, decay=1.0, explor=0.2, q_init=0.0, plus=plus, linear=linear, act_a="learn",
                                act_b="uniform")
        q.update(**one)
        assert q.Q_a[2].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0] and q.Q_b[2].tolist() == [-1.0, 0.0, 0.0, 0.0, 0.0]
        u = 0.0
        for k in range(5):
            u = u + 0.2 * q.Q_a[2][k]
        assert u == 0.2
        low = 0.0 if plus else 0.0 + (0.0 - u)
        top = 0.0 + (1.0 - u)
        assert q.R[0][2].tolist() == [low, top, low, low, low] and top == 0.8
        assert q.Z[0][2].tolist() == [0.0 + 1.0 * 0.2] * 5 and q.updates.tolist() == [0, 0, 1, 0]
        assert (q.n_fallback, q.n_floor, q.n_negative) == (1, 4 if plus else 0, 0 if plus else 4)
        assert policy(q.R[0][2])[0].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0]
        q.update(**one)
        low2 = 0.0 if plus else low + (0.0 - 1.0)
        assert q.R[0][2].tolist() == [low2, top + (1.0 - 1.0), low2, low2, low2]
        w = 2.0 if linear else 1.0
        assert q.Z[0][2].tolist() == [0.2 + w * 0.0, 0.2 + w * 1.0, 0.2 + w * 0.0, 0.2 + w * 0.0, 0.2 + w * 0.0]
        assert average(q.Z[0][2]).tolist() == (q.Z[0][2] / (((((0.0 + 0.2) + (0.2 + w)) + 0.2) + 0.2) + 0.2)).tolist()
        assert (q.n_fallback, q.n_floor, q.n_negative) == (1, 8 if plus else 0, 0 if plus else 8)
        assert q.updates.tolist() == [0, 0, 2, 0] and q.steps == 2 and q.alpha == 1.0
        # nothing else moved: the other states, and the player that does not learn
        rest = [0, 1, 3]
        assert (q.R[0][rest] == 0.0).all() and (q.Z[0][rest] == 0.0).all() and (q.R[1] == 0.0).all() and (q.Z[1] == 0.0).all()
        assert q.visits[2, 5] == 2 and q.visits.sum() == 2
        q.update(obs=[3], act_a=[4], act_b=[2], reward=[0], terminated=[0], next_obs=[2])
        vb = 0.0
        for k in range(5):
            vb = vb + 0.2 * q.Q_b[2][k]
        assert q.Q_a[3].tolist() == [0.0, 0.0, 0.0, 0.0, 0.5 * 1.0]          # not the maximum's doing alone: see B
        assert q.Q_b[3].tolist() == [0.0, 0.0, 0.5 * (float(np.rint(vb * SCALE)) * 2.0 ** -40), 0.0, 0.0] and q.Q_b[3][2] < 0.0
        d = q.derived()
        assert (d["pi_b"] == 0.2).all() and (d["avg_b"] == 0.2).all() and (d["pi_a"][[0, 1]] == 0.2).all()


def test_plus_keeps_the_regrets_at_or_above_plus_zero():
    """under plus no regret is negative, and none is -0.0"""
    rng = np.random.default_rng(3)
    n, nS = 4000, 50
    q = RegretMatchingNumpy(nS, 0.9, q_init=0.5, alpha=0.5, plus=True)
    for _ in range(4):
        q.update(rng.integers(1, nS, n), rng.integers(0, 5, n), rng.integers(0, 5, n), rng.integers(-1, 2, n), rng.integers(0, 2, n),
                 rng.integers(1, nS, n))
    for R in q.R:
        assert (R >= 0.0).all() and not np.signbit(R).any() and (R > 0.0).any()
    assert q.n_floor > 0 and q.n_negative == 0
    assert int(q.visits.sum()) == 4 * n and (q.updates == (q.visits.sum(1) > 0) * np.uint64(4)).all()


def test_with_both_players_fixed_the_tables_are_a_scalar_loop_s():
    """Both players FIXED: R and Z stay zero and the Q tables are what a direct loop gives, a state, a cell and an operation
    at a time, with the bootstrap the definition names: rint(sum_k policy[k] * Q[k] * 2^40) of the previous step."""
    rng = np.random.default_rng(5)
    nS, n, gamma, alpha, decay = 9, 300, 0.9, 0.75, 0.9
    pa, pb = rng.dirichlet(np.ones(5), nS), rng.dirichlet(np.ones(5), nS)
    q = RegretMatchingNumpy(nS, gamma, alpha=alpha, decay=decay, q_init=0.5, act_a=pa, act_b=pb)
    Q = [[[0.0 if s == 0 else 0.5 for _ in range(5)] for s in range(nS)] for _ in range(2)]
    for _ in range(3):
        batch = (rng.integers(1, nS, n), rng.integers(0, 5, n), rng.integers(0, 5, n), rng.integers(-1, 2, n), rng.integers(0, 2, n),
                 rng.integers(0, nS, n))
        q.update(*batch)
        Vq = [[0] * nS, [0] * nS]
        for p, pol in ((0, pa), (1, pb)):
            for s in range(nS):
                v = 0.0
                for k in range(5):
                    v = v + float(pol[s][k]) * Q[p][s][k]
                Vq[p][s] = int(np.rint(v * SCALE))
        for s in range(1, nS):
            for p in (0, 1):
                for k in range(5):
                    c = R = SV = 0
                    for o, a, b, r, term, s2 in zip(*batch):
                        if int(o) == s and int((a, b)[p]) == k:
                            c += 1; R += int(r) if p == 0 else -int(r); SV += 0 if term else Vq[p][int(s2)]
                    if c:
                        m = (float(R) + gamma * (float(SV) * 2.0 ** -40)) / float(c)
                        Q[p][s][k] = Q[p][s][k] + alpha * (m - Q[p][s][k])
        alpha = alpha * decay
        assert q.Q_a.tolist() == Q[0] and q.Q_b.tolist() == Q[1] and q.alpha == alpha
    assert all((x == 0.0).all() for x in q.R + q.Z) and q.n_fallback == 0 and int(q.updates.sum()) > 0


@pytest.mark.parametrize("case", RUN_CASES, ids=RUN_IDS)
def test_the_short_runs_take_every_branch(case):
    w, h, slip, act_a, act_b, plus, linear, max_steps = case
    o, ref = reference_run(*case)
    print("%dx%d slip %g (%s, %s) plus %d linear %d: fallback rows %d, floored %d, negative %d; truncated %d, terminated %d" % (
        w, h, slip, act_a, act_b, plus, linear, ref.n_fallback, ref.n_floor, ref.n_negative, ref.n_truncated, ref.n_terminated))
    assert ref.n_fallback > 0 and (ref.n_floor > 0 if plus else ref.n_negative > 0)
    assert (ref.n_negative == 0) if plus else (ref.n_floor == 0)
    if max_steps == 5:
        assert ref.n_truncated > ref.n_terminated > 0            # truncated-only transitions bootstrap
    s = ref.state()
    assert int(s["visits"].sum()) == N_RUN * T_RUN and s["steps"] == T_RUN and int(s["updates"].max()) <= T_RUN
    assert ((s["updates"] > 0) == (s["visits"].sum(1) > 0)).all()
    if (w, h) == (5, 4) and max_steps == 100:                    # (episodes of five steps do not reach every state)
        assert (s["visits"].sum(1)[1:] > 0).all(), "a live state of 5x4 was never touched"
    for p, name in ((0, act_a), (1, act_b)):
        R, Z = ref.R[p], ref.Z[p]
        if name != "learn":                                     # a player that does not learn leaves R and Z zeros
            assert (R == 0.0).all() and (Z == 0.0).all()
            continue
        assert (R[0] == 0.0).all() and (Z[0] == 0.0).all() and (R[1:] != 0.0).any()
        assert (Z >= 0.0).all() and np.isfinite(R).all() and np.isfinite(Z).all()
        if plus:
            assert (R >= 0.0).all() and not np.signbit(R).any()
        # a step adds one policy row, weighed 1 or n: the row sums of Z are the update counts, or their triangular numbers
        n = s["updates"].astype(np.float64)
        want = n * (n + 1.0) / 2.0 if linear else n
        assert np.abs(Z.sum(1) - want).max() <= 1e-9 * max(1.0, want.max())


# ---- learning ------------------------------------------------------------------------------------------------------------
# the learning run tests/test_gpu_regret_matching.py repeats on the device: self-play from Q = 0, regret matching+
LEARN = dict(width=5, height=4, slip=0.0, gamma=0.9, n=8192, T=500, seed=1994, explor=0.2, q_init=0.0, alpha=1.0, plus=True,
             linear=False)

_LEARNED = {}


def learning_run():
    """(oracle, restatement) of the learning run; computed once and left unchanged"""
    if not _LEARNED:
        c = LEARN
        o = Oracle(c["width"], c["height"], c["slip"], n=c["n"], seed=c["seed"], autoreset=True)
        q = RegretMatchingNumpy(o.nS, c["gamma"], alpha=c["alpha"], decay=0.01 ** (1.0 / c["T"]), explor=c["explor"], q_init=c["q_init"],
                                plus=c["plus"], linear=c["linear"])
        q.run(o, o.reset(), c["T"])
        _LEARNED["run"] = (o, q)
    return _LEARNED["run"]


def mean_gap(lists, pi_a, pi_b, gamma):
    """the exact gap (the best response to pi_a against the best response to pi_b), mean over the live states"""
    return float(np.asarray(br.exploitability(lists, pi_a, pi_b, gamma, 1e-10)["gap"]).reshape(-1, pi_a.shape[0])[0][1:].mean())


def test_the_restatement_learns_in_self_play():
    """Mean over the 760 live states of the exact gap after 500 steps of 8 192 lanes in self-play from Q = 0, alpha 1 -> 0.01,
    explor 0.2, regret matching+, seed 1994, slip 0: the average pair must beat the uniform pair, strictly.  No magic number:
    all three figures are printed (DESIGN §27 has them)."""
    c = LEARN
    o, q = learning_run()
    lists = shapley_lists(Oracle(c["width"], c["height"], c["slip"], n=4, seed=c["seed"], autoreset=True))
    uniform = np.full((o.nS, 5), 0.2)
    d = q.derived()
    g_uniform = mean_gap(lists, uniform, uniform, c["gamma"])
    g_avg = mean_gap(lists, d["avg_a"], d["avg_b"], c["gamma"])
    g_pi = mean_gap(lists, d["pi_a"], d["pi_b"], c["gamma"])
    print("mean exact gap over the live states: uniform pair %.4f, average pair %.4f, current pair %.4f; fallback rows %d, floored %d" % (
        g_uniform, g_avg, g_pi, q.n_fallback, q.n_floor))
    assert (q.visits.sum(1)[1:] > 0).all(), "a live state was never visited"
    assert int(q.visits.sum()) == c["n"] * c["T"] and q.steps == c["T"]
    assert g_avg < g_uniform
