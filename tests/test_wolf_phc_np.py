"""The numpy restatement of the policy hill-climbers (tests/wolf_phc_np.py) does what the definition says on a hand case, keeps
its rows policies, takes every branch of the policy step in the short runs the GPU tests use, and learns: against a uniform
player A, player B's hill-climbed policy approaches the value of the exact best response to that opponent (the CPU pair
evaluation and best-response iteration of tests/best_response_np.py).  tests/test_gpu_wolf_phc.py pins the device to this
restatement bit for bit, so this guards the yardstick where there is no GPU."""
import os
import sys

import numpy as np
import pytest

from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_response_np as br  # noqa: E402
from minimax_q_np import shapley_lists  # noqa: E402
from wolf_phc_np import WolfPHCNumpy  # noqa: E402

EPS = 2.0 ** -52
GAMMA = 0.9

# ---- the short runs tests/test_gpu_wolf_phc.py repeats on the device ---------------------------------------------------------
N_RUN, T_RUN, SEED = 8192 + 3, 60, 1994
RUN_KW = dict(explor=0.2, decay=0.99, delta_win=0.1, delta_lose=0.4)
# width, height, slip, act_a, act_b, further parameters
RUN_CASES = [(5, 4, 0.0, "learn", "uniform", {}),
             (5, 4, 0.2, "learn", "learn", {"delta_decay": 0.98}),
             (7, 5, 0.3, "dirichlet", "learn", {}),
             (11, 7, 0.2, "uniform", "learn", {})]
RUN_IDS = ["5x4 slip 0 learn-uniform", "5x4 slip 0.2 learn-learn decaying deltas", "7x5 slip 0.3 fixed-learn", "11x7 slip 0.2 uniform-learn"]


def act(name, nS):
    if isinstance(name, str) and name == "dirichlet":
        return np.random.default_rng(11).dirichlet(np.ones(5), nS)
    return name


_REFERENCE = {}


def reference_run(w, h, slip, act_a, act_b, extra=(), T=T_RUN, n=N_RUN):
    """(oracle, restatement) after T steps; computed once per case and left unchanged"""
    key = (w, h, slip, act_a, act_b, tuple(sorted(dict(extra).items())), T, n)
    if key not in _REFERENCE:
        o = Oracle(w, h, slip, n=n, seed=SEED, autoreset=True)
        kw = dict(RUN_KW); kw.update(dict(extra))
        ref = WolfPHCNumpy(o.nS, GAMMA, act_a=act(act_a, o.nS), act_b=act(act_b, o.nS), **kw)
        ref.run(o, o.reset(), T)
        _REFERENCE[key] = (o, ref)
    return _REFERENCE[key]


def row_sum_bounds(updates):
    """How far a row's sum may be from 1 after n policy steps, from the arithmetic alone.  A step of pi rounds at most four
    subtractions, four additions into `moved` and one into pi[g], each by at most EPS / 2 on values <= 1: 4.5 EPS; summing the
    row rounds four times more.  avg[k] + (pi[k] - avg[k]) / n rounds three times per entry, 7.5 EPS a row, and carries the
    mean of the deviations pi had.  So |sum(pi) - 1| <= 5 EPS (n + 1) and |sum(avg) - 1| <= 13 EPS (n + 1)."""
    n = np.asarray(updates).astype(np.float64) + 1.0
    return 5.0 * EPS * n, 13.0 * EPS * n


def assert_rows_are_policies(s):
    for p in "ab":
        lim_pi, lim_avg = row_sum_bounds(s["updates"])
        assert (s["pi_" + p] >= 0.0).all() and (s["avg_" + p] >= 0.0).all()
        assert (np.abs(s["pi_" + p].sum(1) - 1.0) <= lim_pi).all(), np.abs(s["pi_" + p].sum(1) - 1.0).max()
        assert (np.abs(s["avg_" + p].sum(1) - 1.0) <= lim_avg).all(), np.abs(s["avg_" + p].sum(1) - 1.0).max()


def test_two_updates_by_hand():
    """one state, alpha = 1, the Q row (0, 1, 0, 0, 0) after the first update.  First update: the state's first touch, so avg
    stays and ep == ea: the delta_lose branch, d = 0.15, nothing clamps.  Second: n = 2 moves avg half way, ep > ea: the
    delta_win branch at dscale = 0.5, d = 0.0625 > pi[k] = 0.05: every other entry is clamped to exactly 0."""
    q = WolfPHCNumpy(4, 0.5, alpha=1.0, decay=1.0, explor=0.2, q_init=0.0, delta_win=0.5, delta_lose=0.6, delta_decay=0.5,
                     act_a="learn", act_b="uniform")
    one = dict(obs=[2], act_a=[1], act_b=[0], reward=[1], terminated=[1], next_obs=[0])
    q.update(**one)
    assert q.Q_a[2].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0] and q.Q_b[2].tolist() == [-1.0, 0.0, 0.0, 0.0, 0.0]
    assert q.updates.tolist() == [0, 0, 1, 0] and q.avg[0][2].tolist() == [0.2] * 5
    d = (0.6 * 1.0) / 4.0
    low = 0.2 - d
    moved = 0.0
    for _ in range(4):
        moved = moved + d
    top = 0.2 + moved
    assert q.pi[0][2].tolist() == [low, top, low, low, low]
    assert (q.n_win, q.n_lose, q.n_clamp) == (0, 1, 0) and q.dscale == 0.5 and q.alpha == 1.0 and q.steps == 1
    q.update(**one)
    assert q.Q_a[2].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0] and q.updates.tolist() == [0, 0, 2, 0]
    avg_low, avg_top = 0.2 + (low - 0.2) / 2.0, 0.2 + (top - 0.2) / 2.0
    assert q.avg[0][2].tolist() == [avg_low, avg_top, avg_low, avg_low, avg_low]
    assert top > avg_top and (0.5 * 0.5) / 4.0 > low > 0.0
    moved = 0.0
    for _ in range(4):
        moved = moved + low
    assert q.pi[0][2].tolist() == [0.0, top + moved, 0.0, 0.0, 0.0]
    assert (q.n_win, q.n_lose, q.n_clamp) == (1, 1, 4) and q.dscale == 0.25 and q.steps == 2
    # nothing else moved: the other states, and the player that does not learn
    rest = [0, 1, 3]
    assert (q.pi[0][rest] == 0.2).all() and (q.avg[0][rest] == 0.2).all() and (q.pi[1] == 0.2).all() and (q.avg[1] == 0.2).all()
    assert q.visits[2, 5] == 2 and q.visits.sum() == 2
    s = q.state()
    assert s["V_a"][2] == 1.0 and s["V_b"][2] == 0.0 and s["dscale"] == 0.25


def test_plain_phc_ignores_the_branch():
    """delta_win == delta_lose: both branches step alike, so the run does not depend on avg"""
    rng = np.random.default_rng(3)
    n = 4000
    batch = (rng.integers(1, 50, n), rng.integers(0, 5, n), rng.integers(0, 5, n), np.zeros(n, np.int64), np.zeros(n, np.uint8),
             rng.integers(1, 50, n))
    a = WolfPHCNumpy(50, 0.9, q_init=0.5, delta_win=0.04, delta_lose=0.04)
    b = WolfPHCNumpy(50, 0.9, q_init=0.5, delta_win=0.04, delta_lose=0.04)
    b.avg[0][:] = np.eye(5)[2]                                 # another average: another branch, the same step
    for _ in range(3):
        a.update(*batch); b.update(*batch)
    assert a.pi[0].tobytes() == b.pi[0].tobytes() and a.avg[0].tobytes() != b.avg[0].tobytes()


@pytest.mark.parametrize("case", RUN_CASES, ids=RUN_IDS)
def test_the_short_runs_take_every_branch_and_keep_rows_policies(case):
    w, h, slip, act_a, act_b, extra = case
    o, ref = reference_run(w, h, slip, act_a, act_b, extra)
    print("%dx%d slip %g (%s, %s): ep > ea %d times, else %d times, min() clamped %d times" % (
        w, h, slip, act_a, act_b, ref.n_win, ref.n_lose, ref.n_clamp))
    assert ref.n_win > 0 and ref.n_lose > 0 and ref.n_clamp > 0
    s = ref.state()
    assert_rows_are_policies(s)
    assert int(s["visits"].sum()) == N_RUN * T_RUN and s["steps"] == T_RUN and int(s["updates"].max()) <= T_RUN
    assert (s["updates"] > 0).sum() == (s["visits"].sum(1) > 0).sum()
    # a player that does not learn keeps pi and avg, bit for bit
    for p, name in ((0, act_a), (1, act_b)):
        if name != "learn":
            const = np.full((o.nS, 5), 0.2) if name == "uniform" else act(name, o.nS)
            assert ref.pi[p].tobytes() == const.tobytes() and ref.avg[p].tobytes() == const.tobytes()
        else:
            assert (ref.pi[p][1:] != 0.2).any() and (ref.pi[p][0] == 0.2).all() and (ref.avg[p][0] == 0.2).all()


# ---- learning ------------------------------------------------------------------------------------------------------------
# the learning run of tests/test_gpu_wolf_phc.py: player A FIXED uniform, player B LEARN
LEARN = dict(width=5, height=4, slip=0.0, gamma=0.9, n=65536, T=3000, seed=1994, explor=0.2, q_init=0.0, alpha=1.0,
             delta_win=0.01, delta_lose=0.04, delta_decay=1.0)
# Mean over the 760 live states of  V(uniform, pi_b) - V(uniform, B's exact best response)  (player A's value: >= 0 up to
# theta), measured with this restatement; the same for the average policy avg_b, and the Q side |-V_b - V(best response)|:
#   seed, slip      pi_b mean   (max)        avg_b mean     Q side mean
#   1994, 0         0.001213    (0.0954)     0.012242       0.002592
#   1,    0         0.001161    (0.0582)     0.012154       0.002521
#   2,    0         0.001226    (0.0662)     0.012062       0.002266
#   7,    0.2       0.000935    (0.0436)     0.012517       0.002132
# Every live state was visited in every run and every difference was >= -1e-9.  The maximum is carried by a few rarely
# visited states and is noisy, so the mean is what is asserted: twice the worst of the four.
BOUND = 2 * 0.001226


def learning_grade(lists, uniform, pi_b, want, gamma):
    return (br.evaluate(lists, uniform, pi_b, gamma, 1e-10)[0][0] - want)[1:]


def test_the_restatement_learns_a_best_response_policy():
    """mean over live states of V(uniform, pi_b) - V(uniform, best response) after 3 000 steps of 65 536 lanes from Q = 0,
    seed 1994, slip 0: measured 0.001213 (max 0.0954); it and the maximum are printed below."""
    c = LEARN
    o = Oracle(c["width"], c["height"], c["slip"], n=c["n"], seed=c["seed"], autoreset=True)
    uniform = np.full((o.nS, 5), 0.2)
    lists = shapley_lists(Oracle(c["width"], c["height"], c["slip"], n=4, seed=c["seed"], autoreset=True))
    want = br.best_response(lists, uniform, 0, c["gamma"], 1e-10)[1][0]          # B answers a uniform A
    q = WolfPHCNumpy(o.nS, c["gamma"], alpha=c["alpha"], decay=0.01 ** (1.0 / c["T"]), explor=c["explor"], q_init=c["q_init"],
                     delta_win=c["delta_win"], delta_lose=c["delta_lose"], delta_decay=c["delta_decay"], act_a=uniform, act_b="learn")
    q.run(o, o.reset(), c["T"])
    s = q.state()
    d = learning_grade(lists, uniform, s["pi_b"], want, c["gamma"])
    lag = learning_grade(lists, uniform, s["avg_b"], want, c["gamma"])
    print("pi_b: mean %.6f  max %.6f  min %.3g;  avg_b: mean %.6f;  Q side: mean %.6f;  branches %d / %d / %d" % (
        d.mean(), d.max(), d.min(), lag.mean(), np.abs(-s["V_b"] - want)[1:].mean(), q.n_win, q.n_lose, q.n_clamp))
    assert (q.visits.sum(1)[1:] > 0).all(), "a live state was never visited"
    assert int(q.visits.sum()) == c["n"] * c["T"] and int(q.updates.max()) <= c["T"]
    assert_rows_are_policies(s)
    assert s["pi_a"].tobytes() == uniform.tobytes() and s["avg_a"].tobytes() == uniform.tobytes()
    assert d.min() >= -1e-9
    assert d.mean() <= BOUND
