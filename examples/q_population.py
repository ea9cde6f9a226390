"""Many independent Q-learners at once, a learner per lane (SoccerBatch.q_population): Littman (1994) trains ONE learner from one
stream of experience and reports several runs; Bowling & Veloso (2002) report the mean over 50 trials.  Here a population of
QR learners (greedy A against a uniform B) and one of QQ learners (both greedy) train in one run each, every member with its
own tables and its own Philox stream, and the exact gap of every member's greedy pair — how badly the best possible opponent
beats it (QPopulation.exploitability) — is printed as quartiles over the members: a distribution instead of one seed's figure.
A third population sweeps explor over its members in the same run.  Prints tables; asserts nothing.

    python examples/q_population.py [steps] [members] [seed]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_soccer_littman94_amd import VectorSoccerEnv  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
N = int(sys.argv[2]) if len(sys.argv) > 2 else 512
SEED = int(sys.argv[3]) if len(sys.argv) > 3 else 1994
GAMMA = 0.9
KW = dict(alpha=1.0, decay=0.01 ** (1.0 / max(T, 1)), q_init=0.0)


def train(name, explor=0.2, **how):
    env = VectorSoccerEnv(N, width=5, height=4, slip_prob=0.0, seed=SEED, autoreset=True)
    env.reset()
    pop = env.q_population(GAMMA, explor=explor, **how, **KW)
    pop.run(T)
    gap = pop.exploitability(theta=1e-8)["gap"][:, 1:].mean(1)       # per member: the mean over the live states
    print("trained %-6s %d members x %d steps, training episodes (-1, 0, +1) %s" % (name, N, T, env.episode_histogram().tolist()))
    pop.close()
    env.close()
    return gap


def quartiles(x):
    return "min %.4f  q1 %.4f  median %.4f  q3 %.4f  max %.4f" % tuple(np.percentile(x, [0, 25, 50, 75, 100]))


qr = train("QR", act_a="greedy", act_b="uniform")
qq = train("QQ", act_a="greedy", act_b="greedy")
print("\nexact gap of a member's greedy pair, mean over the live states; quartiles over the %d members" % N)
print("QR  " + quartiles(qr))
print("QQ  " + quartiles(qq))

# a sweep in the same run: explor differs from member to member, everything else is shared
values = np.array([0.05, 0.1, 0.2, 0.4])
explor = values[np.arange(N) % values.size]
sweep = train("QQ", explor=explor, act_a="greedy", act_b="greedy")
print("\nQQ, explor swept over the members of one population")
for v in values:
    print("explor %.2f (%3d members)  " % (v, int((explor == v).sum())) + quartiles(sweep[explor == v]))
