"""The vectorised numpy restatement of the population of policy hill-climbers (tests/wolf_population_np.py) is n separate
one-actor WoLF-PHC learners (tests/wolf_phc_np.py, member i fed lane i's transitions through update()) bit for bit, does what
the definition says on a hand case, takes every branch of the policy step in the short runs the GPU tests use, and learns:
against a uniform player A every member's hill-climbed pi_b approaches the value of the exact best response
(tests/best_response_np.py).  tests/test_gpu_wolf_population.py pins the device to this restatement bit for bit, so this
guards the yardstick where there is no GPU."""
import os
import sys
import time

import numpy as np
import pytest

from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import best_response_np as br  # noqa: E402
from minimax_q_np import shapley_lists  # noqa: E402
from wolf_phc_np import WolfPHCNumpy  # noqa: E402
from wolf_population_np import WolfPopulationNumpy, assert_wolf_population_equal  # noqa: E402

GAMMA = 0.9

# ---- the short runs tests/test_gpu_wolf_population.py repeats on the device --------------------------------------------------
T_RUN, SEED = 60, 1994
RUN_KW = dict(explor=0.2, decay=0.99, delta_win=0.1, delta_lose=0.4)
# width, height, slip, act_a, act_b, members, max_steps, further parameters.  Member counts: a single lane, a ragged wave,
# a ragged workgroup.  Every case starts from a loaded state (WolfPopulationNumpy.load: Q uniform in [-1, 1], Dirichlet pi and
# avg, small update counts): from pi = 0.2 and Q = q_init sixty single-sample steps would mostly see ep == ea.
RUN_CASES = [(5, 4, 0.0, "learn", "uniform", 1, 100, {}),
             (5, 4, 0.0, "learn", "uniform", 67, 100, {}),
             (5, 4, 0.2, "learn", "learn", 259, 100, {"delta_decay": 0.98}),
             (7, 5, 0.3, "dirichlet", "learn", 67, 100, {}),
             (11, 7, 0.2, "uniform", "learn", 67, 100, {}),
             (5, 4, 0.2, "learn", "learn", 259, 6, {})]
RUN_IDS = ["5x4 slip 0 learn-uniform 1", "5x4 slip 0 learn-uniform 67", "5x4 slip 0.2 learn-learn decaying deltas 259",
           "7x5 slip 0.3 fixed per member-learn 67", "11x7 slip 0.2 uniform-learn 67", "5x4 slip 0.2 learn-learn truncating 259"]


def act(name, n, nS):
    """'dirichlet': a fixed policy per member"""
    if isinstance(name, str) and name == "dirichlet":
        return np.random.default_rng(11).dirichlet(np.ones(5), (n, nS))
    return name


_REFERENCE = {}


def reference_run(w, h, slip, act_a, act_b, n, max_steps=100, extra=(), T=T_RUN, seed=SEED):
    """(oracle, restatement, the loaded state it started from) after T steps; computed once per case and left unchanged"""
    key = (w, h, slip, act_a, act_b, n, max_steps, tuple(sorted(dict(extra).items())), T, seed)
    if key not in _REFERENCE:
        o = Oracle(w, h, slip, n=n, seed=seed, autoreset=True, max_steps=max_steps)
        kw = dict(RUN_KW); kw.update(dict(extra))
        ref = WolfPopulationNumpy(n, o.nS, GAMMA, act_a=act(act_a, n, o.nS), act_b=act(act_b, n, o.nS), **kw)
        start = ref.load(np.random.default_rng(seed + n))
        ref.run(o, o.reset(), T)
        _REFERENCE[key] = (o, ref, start)
    return _REFERENCE[key]


@pytest.mark.parametrize("case", RUN_CASES, ids=RUN_IDS)
def test_the_short_runs_take_every_branch(case):
    w, h, slip, act_a, act_b, n, max_steps, extra = case
    o, ref, start = reference_run(w, h, slip, act_a, act_b, n, max_steps, extra)
    print("%dx%d slip %g (%s, %s), %d members: ep > ea %d times, else %d times, min() clamped %d times; s' == s %d, terminated %d, "
          "truncated only %d" % (w, h, slip, act_a, act_b, n, ref.n_win, ref.n_lose, ref.n_clamp, ref.n_same, ref.n_terminated,
                                 ref.n_truncated_only))
    assert ref.n_win > 0 and ref.n_lose > 0 and ref.n_clamp > 0
    assert ref.n_left_out == 0 and ref.steps == T_RUN
    if n > 1:
        assert ref.n_same > 0
    if max_steps == 6:
        assert ref.n_truncated_only > 0 and ref.n_terminated > 0
    s = ref.state()
    assert int((s["updates"] - start["updates"]).sum()) == n * T_RUN
    for p, name in ((0, act_a), (1, act_b)):            # a player that does not learn keeps pi and avg, bit for bit
        k = "ab"[p]
        if name != "learn":
            assert s["pi_" + k].tobytes() == start["pi_" + k].tobytes() and s["avg_" + k].tobytes() == start["pi_" + k].tobytes()
        else:
            assert (s["pi_" + k] >= 0.0).all() and np.abs(s["pi_" + k][:, 1:].sum(2) - 1.0).max() < 1e-12
            assert s["pi_" + k].tobytes() != start["pi_" + k].tobytes()


# ---- the vectorised restatement is n separate learners ----------------------------------------------------------------------
@pytest.mark.parametrize("modes", [("learn", "learn"), ("fixed", "learn")], ids=["learn-learn", "fixed per member-learn"])
def test_the_vectorised_restatement_is_n_separate_learners_bit_for_bit(modes):
    """5x4, slip 0.2, 33 members, 200 steps, max_steps = 6 so that episodes truncate; per-member arrays for all seven
    hyperparameters; a fixed player A has a policy per member"""
    n, T = 33, 200
    rng = np.random.default_rng(5)
    hyper = dict(alpha=rng.uniform(0.3, 1.0, n), decay=rng.uniform(0.95, 1.0, n), explor=rng.uniform(0.05, 0.6, n),
                 delta_win=rng.uniform(0.01, 0.2, n), delta_lose=rng.uniform(0.2, 0.8, n), delta_decay=rng.uniform(0.97, 1.0, n))
    gam = rng.uniform(0.5, 0.95, n)
    o = Oracle(5, 4, 0.2, n=n, seed=1994, autoreset=True, max_steps=6)
    fixed = rng.dirichlet(np.ones(5), (n, o.nS))
    acts = lambda i: tuple((fixed if i is None else fixed[i]) if m == "fixed" else m for m in modes)  # noqa: E731
    pop = WolfPopulationNumpy(n, o.nS, gam, q_init=0.3, act_a=acts(None)[0], act_b=acts(None)[1], **hyper)
    solo = [WolfPHCNumpy(o.nS, gam[i], q_init=0.3, act_a=acts(i)[0], act_b=acts(i)[1], **{k: v[i] for k, v in hyper.items()}) for i in range(n)]
    obs = o.reset()
    for _ in range(T):
        rows = [np.stack([q._table(p)[s] for q, s in zip(solo, obs)]) for p in (0, 1)]
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
    want = {"Q_a": np.stack([q.Q_a for q in solo]), "Q_b": np.stack([q.Q_b for q in solo]),
            "pi_a": np.stack([q.pi[0] for q in solo]), "pi_b": np.stack([q.pi[1] for q in solo]),
            "avg_a": np.stack([q.avg[0] for q in solo]), "avg_b": np.stack([q.avg[1] for q in solo]),
            "updates": np.stack([q.updates for q in solo]), "alpha": np.array([q.alpha for q in solo]),
            "dscale": np.array([q.dscale for q in solo]), "steps": solo[0].steps}
    assert_wolf_population_equal(pop.state(), want)
    assert (pop.n_win, pop.n_lose, pop.n_clamp) == tuple(sum(getattr(q, k) for q in solo) for k in ("n_win", "n_lose", "n_clamp"))
    assert pop.steps == T and pop.n_lose > 0 and (pop.pi[1] != 0.2).sum() > n
    if modes[0] == "fixed":
        assert pop.pi[0].tobytes() == fixed.tobytes() and pop.avg[0].tobytes() == fixed.tobytes()
    # run() is the same loop: a second population driven by run() on a second oracle ends in the same bits
    o2 = Oracle(5, 4, 0.2, n=n, seed=1994, autoreset=True, max_steps=6)
    pop2 = WolfPopulationNumpy(n, o2.nS, gam, q_init=0.3, act_a=acts(None)[0], act_b=acts(None)[1], **hyper)
    pop2.run(o2, o2.reset(), T)
    assert_wolf_population_equal(pop2.state(), pop.state())
    assert (pop2.n_same, pop2.n_terminated, pop2.n_truncated_only, pop2.n_left_out) == (pop.n_same, pop.n_terminated, pop.n_truncated_only, 0)


def test_one_member_two_steps_by_hand():
    """tests/test_wolf_phc_np.py's hand case as member 1 of three: alpha = 1, the Q row (0, 1, 0, 0, 0) after the first update.
    First update: the state's first touch, so avg stays and ep == ea: the delta_lose branch, d = 0.15, nothing clamps.  Second:
    n = 2 moves avg half way, ep > ea: the delta_win branch at dscale = 0.5, d = 0.0625 > pi[k] = 0.05: every other entry is
    clamped to exactly 0.  Member 0 has other deltas and is left out of the second update; member 2 is never kept."""
    q = WolfPopulationNumpy(3, 4, 0.5, alpha=1.0, decay=1.0, explor=0.2, q_init=0.0, delta_win=[0.1, 0.5, 0.5], delta_lose=[0.2, 0.6, 0.6],
                            delta_decay=[1.0, 0.5, 0.25], act_a="learn", act_b="uniform")
    one = dict(obs=[2, 2, 3], act_a=[1, 1, 0], act_b=[0, 0, 0], reward=[1, 1, 0], terminated=[1, 1, 0], next_obs=[0, 0, 1])
    q.update(keep=[True, True, False], **one)
    assert q.Q_a[1, 2].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0] and q.Q_b[1, 2].tolist() == [-1.0, 0.0, 0.0, 0.0, 0.0]
    assert q.updates.tolist() == [[0, 0, 1, 0], [0, 0, 1, 0], [0, 0, 0, 0]] and q.avg[0][1, 2].tolist() == [0.2] * 5
    d = (0.6 * 1.0) / 4.0
    low = 0.2 - d
    moved = 0.0
    for _ in range(4):
        moved = moved + d
    top = 0.2 + moved
    assert q.pi[0][1, 2].tolist() == [low, top, low, low, low]
    d0 = (0.2 * 1.0) / 4.0
    assert q.pi[0][0, 2].tolist() == [0.2 - d0, 0.2 + (((0.0 + d0) + d0) + d0 + d0), 0.2 - d0, 0.2 - d0, 0.2 - d0]
    assert (q.n_win, q.n_lose, q.n_clamp) == (0, 2, 0) and q.dscale.tolist() == [1.0, 0.5, 0.25] and q.steps == 1
    first = q.pi[0][0].copy()
    q.update(keep=[False, True, False], **one)
    assert q.updates.tolist() == [[0, 0, 1, 0], [0, 0, 2, 0], [0, 0, 0, 0]]
    avg_low, avg_top = 0.2 + (low - 0.2) / 2.0, 0.2 + (top - 0.2) / 2.0
    assert q.avg[0][1, 2].tolist() == [avg_low, avg_top, avg_low, avg_low, avg_low]
    assert top > avg_top and (0.5 * 0.5) / 4.0 > low > 0.0
    moved = 0.0
    for _ in range(4):
        moved = moved + low
    assert q.pi[0][1, 2].tolist() == [0.0, top + moved, 0.0, 0.0, 0.0]
    assert (q.n_win, q.n_lose, q.n_clamp) == (1, 2, 4) and q.dscale.tolist() == [1.0, 0.25, 0.0625] and q.steps == 2
    # nothing else moved: the member left out, the member never kept, the other states, the player that does not learn
    assert q.pi[0][0].tobytes() == first.tobytes() and (q.pi[0][2] == 0.2).all() and (q.Q_a[2] == 0.0).all()
    assert (q.pi[0][1, [0, 1, 3]] == 0.2).all() and (q.avg[0][1, [0, 1, 3]] == 0.2).all() and (q.pi[1] == 0.2).all() and (q.avg[1] == 0.2).all()


# ---- learning ------------------------------------------------------------------------------------------------------------
# the learning run of tests/test_gpu_wolf_population.py: player A FIXED uniform, player B LEARN, a learner per lane, alpha 1 -> 0.01
LEARN = dict(width=5, height=4, slip=0.0, gamma=0.9, n=64, T=75000, seed=1994, explor=0.2, q_init=0.0, alpha=1.0,
             delta_win=0.01, delta_lose=0.04, delta_decay=1.0)
# T = 75 000: a step of this restatement costs 0.58 ms, so the run takes 44 s on one core and the test stays under a minute.
# Population mean (over the 64 members; min .. max member in brackets) of the mean over the 760 live states, measured with this
# restatement (learning_run below), of
#   policy side  V(uniform, pi_b) - V(uniform, B's exact best response)     (player A's value; how DESIGN section 13 grades)
#   Q side       |-V_b - V(uniform, B's exact best response)|               (how DESIGN section 14 grades)
#   seed, slip     policy side                         Q side
#   1994, 0        0.312553  (0.256594 .. 0.397877)    0.237436  (0.189594 .. 0.305035)
#   1,    0        0.303673  (0.251382 .. 0.365507)    0.230259  (0.185018 .. 0.289160)
#   2,    0.2      0.293434  (0.262654 .. 0.346214)    0.202800  (0.171930 .. 0.250694)
#   7,    0.2      0.293794  (0.246339 .. 0.351697)    0.202343  (0.164543 .. 0.244724)
#   untrained      0.600620 at slip 0, 0.508818 at 0.2 (pi_b uniform)      0.606169 at slip 0, 0.521389 at 0.2 (V_b = 0)
# One learner sees each state about a hundred times in 75 000 steps and a policy row moves by at most delta_lose / 4 = 0.01 per
# visit, so pi_b is about half way.  Twice the worst policy-side figure (0.625) does NOT lie below the untrained 0.6006, so at this
# budget that grade would not show learning; as section 14 did, the Q side is what is asserted: twice the worst of the four
# (section 12's rule), 0.474872, lies below the untrained 0.606169.
BOUND = 2 * 0.237436


def learning_run(seed, slip, T=LEARN["T"], n=LEARN["n"], policy_side=False):
    """(the population after T steps, per-member Q-side error, the untrained Q-side figure[, per-member policy-side
    figure, the untrained one])"""
    c = LEARN
    o = Oracle(c["width"], c["height"], slip, n=n, seed=seed, autoreset=True)
    uniform = np.full((o.nS, 5), 0.2)
    lists = shapley_lists(Oracle(c["width"], c["height"], slip, n=4, seed=seed, autoreset=True))
    want = br.best_response(lists, uniform, 0, c["gamma"], 1e-10)[1][0]          # B answers a uniform A
    q = WolfPopulationNumpy(n, o.nS, c["gamma"], alpha=c["alpha"], decay=0.01 ** (1.0 / T), explor=c["explor"], q_init=c["q_init"],
                            delta_win=c["delta_win"], delta_lose=c["delta_lose"], delta_decay=c["delta_decay"], act_a=uniform, act_b="learn")
    q.run(o, o.reset(), T)
    out = (q, np.abs(-q.Q_b.max(2) - want)[:, 1:].mean(1), np.abs(0.0 - want)[1:].mean())
    if policy_side:
        every = np.ascontiguousarray(np.broadcast_to(uniform, (n, o.nS, 5)))
        out += ((br.evaluate(lists, every, q.pi[1], c["gamma"], 1e-10)[0] - want)[:, 1:].mean(1),
                (br.evaluate(lists, uniform, uniform, c["gamma"], 1e-10)[0][0] - want)[1:].mean())
    return out


def test_the_restatement_learns_the_best_response_values():
    c = LEARN
    t0 = time.perf_counter()
    q, err, untrained = learning_run(c["seed"], c["slip"])
    print("A uniform, B learns, %d members x %d steps, seed %d: Q side, population mean %.6f (members %.6f .. %.6f), untrained %.6f; "
          "branches %d / %d / %d; %.1f s" % (c["n"], c["T"], c["seed"], err.mean(), err.min(), err.max(), untrained, q.n_win, q.n_lose,
                                             q.n_clamp, time.perf_counter() - t0))
    assert q.steps == c["T"] and np.abs(q.alpha - 0.01).max() < 1e-9
    assert q.n_left_out == 0 and q.n_same > 0 and q.n_terminated > 0 and q.n_win > 0 and q.n_lose > 0 and q.n_clamp > 0
    assert (q.pi[0] == 0.2).all() and (q.pi[1] >= 0.0).all() and np.abs(q.pi[1][:, 1:].sum(2) - 1.0).max() < 1e-9
    assert BOUND < untrained                    # the bound shows learning
    assert err.mean() <= BOUND
