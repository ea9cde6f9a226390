"""Regret matchers, a learner per lane (SoccerBatch.regret_population): regret matching per state with Q-values for
counterfactual values (Hart & Mas-Colell 2000; the local no-regret learner of Kash, Sullins & Hofmann 2020), the dynamic behind
CFR and CFR+.  Populations train in self-play (both players learn) in one run each: regret matching+ with plain averaging,
regret matching+ with linear averaging, and plain regret matching.  For every member the exact gap — how badly the best
possible opponent beats the pair (RegretPopulation.exploitability) — of its AVERAGE policies (the pair that carries the
no-regret guarantee) and of its current policies is printed as quartiles over the members, beside a wolf_population trained
with the same seed for the same steps.  Prints tables; asserts nothing.

    python examples/regret_population.py [steps] [members] [seed]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_soccer_littman94_amd import VectorSoccerEnv  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
N = int(sys.argv[2]) if len(sys.argv) > 2 else 256
SEED = int(sys.argv[3]) if len(sys.argv) > 3 else 1994
GAMMA = 0.9
KW = dict(alpha=1.0, decay=0.01 ** (1.0 / max(T, 1)), q_init=0.0, explor=0.2)


def mean_gap(e):
    return e["gap"][:, 1:].mean(1)                 # per member: the mean over the live states


def train(kind, name, **how):
    """-> (per-member gap of the average pair, of the current pair)"""
    env = VectorSoccerEnv(N, width=5, height=4, slip_prob=0.0, seed=SEED, autoreset=True)
    env.reset()
    pop = getattr(env, kind)(GAMMA, **how, **KW)
    pop.run(T)
    gaps = mean_gap(pop.exploitability("avg", theta=1e-8)), mean_gap(pop.exploitability("pi", theta=1e-8))
    print("trained %-18s %-28s %d members x %d steps, training episodes (-1, 0, +1) %s" % (kind, name, N, T, env.episode_histogram().tolist()))
    pop.close()
    env.close()
    return gaps


def quartiles(x):
    return "min %.4f  q1 %.4f  median %.4f  q3 %.4f  max %.4f" % tuple(np.percentile(x, [0, 25, 50, 75, 100]))


rows = [("regret matching+", train("regret_population", "plus", plus=True, linear=False)),
        ("regret matching+, linear", train("regret_population", "plus, linear averaging", plus=True, linear=True)),
        ("regret matching", train("regret_population", "plain", plus=False, linear=False)),
        ("WoLF-PHC", train("wolf_population", "delta_win 0.01, delta_lose 0.04"))]

print("\nself-play; exact gap of a member's pair of policies, mean over the live states; quartiles over the %d members" % N)
for name, (avg, pi) in rows:
    print("(%s)" % name)
    print("  avg  " + quartiles(avg))
    print("  pi   " + quartiles(pi))
