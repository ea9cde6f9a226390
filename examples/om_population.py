"""Opponent-modelling Q-learners, a learner per lane (SoccerBatch.om_population): the learner that sees the other player's
action, counts it, and answers the counted frequencies greedily over a joint-action table (Uther & Veloso 1997; the
joint-action learner of Claus & Boutilier 1998) — in self-play, fictitious play in a Markov game.  Three populations train in
one run each: greedy A against a uniform B, both greedy (self-play), and a challenger B against a fixed policy of A (the
greedy policy of member 0 of the first population).  For every member the exact gap — how badly the best possible opponent
beats the pair (OpponentModelPopulation.exploitability) — of its greedy policies and of its MODELS (the normalised counts:
what each player has seen the other play) is printed as quartiles over the members, beside a q_population trained with the
same seed and steps.  Prints tables; asserts nothing.

    python examples/om_population.py [steps] [members] [seed]
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
    """-> (per-member gap of the greedy pair, of the models or None, member 0's greedy pi_a)"""
    env = VectorSoccerEnv(N, width=5, height=4, slip_prob=0.0, seed=SEED, autoreset=True)
    env.reset()
    pop = getattr(env, kind)(GAMMA, **how, **KW)
    pop.run(T)
    if kind == "om_population":
        gaps = mean_gap(pop.exploitability("greedy", theta=1e-8)), mean_gap(pop.exploitability("model", theta=1e-8))
    else:
        gaps = mean_gap(pop.exploitability(theta=1e-8)), None
    pi_a = pop.read(0, 1)["pi_a"][0]
    print("trained %-14s %-18s %d members x %d steps, training episodes (-1, 0, +1) %s" % (kind, name, N, T, env.episode_histogram().tolist()))
    pop.close()
    env.close()
    return gaps + (pi_a,)


def quartiles(x):
    return "min %.4f  q1 %.4f  median %.4f  q3 %.4f  max %.4f" % tuple(np.percentile(x, [0, 25, 50, 75, 100]))


rows = []
frozen = None
for name, how in (("greedy, uniform", dict(act_a="greedy", act_b="uniform")), ("greedy, greedy", dict(act_a="greedy", act_b="greedy")),
                  ("fixed, greedy", None)):
    if how is None:                                 # the challenger: B learns against member 0's greedy policy of the first run
        how = dict(act_a=frozen, act_b="greedy")
    om = train("om_population", name, **how)
    q = train("q_population", name, **how)
    frozen = om[2] if frozen is None else frozen
    rows.append((name, om, q))

print("\nexact gap of a member's pair of policies, mean over the live states; quartiles over the %d members" % N)
for name, om, q in rows:
    print("(%s)" % name)
    print("  om_population, greedy  " + quartiles(om[0]))
    print("  om_population, models  " + quartiles(om[1]))
    print("  q_population,  greedy  " + quartiles(q[0]))
