"""Littman (1994)'s experiment on this pitch as a distribution over many runs, a learner per lane
(SoccerBatch.minimax_q_population): n minimax-Q learners train against a random opponent (MR) and n in self-play (MM), every
member with its own table, strategies and Philox stream.  For each population the quartiles over the members of
max |V - V*| on the live states (V* from planners.minimax_value_iteration) and of the exact gap of pi_a — how far the best
possible opponent pushes player A's strategy below the game's value, mean over the live states — are printed.  Prints tables;
asserts nothing.

    python examples/minimax_q_population.py [steps] [members] [seed]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_soccer_littman94_amd import VectorSoccerEnv, planners  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
N = int(sys.argv[2]) if len(sys.argv) > 2 else 512
SEED = int(sys.argv[3]) if len(sys.argv) > 3 else 1994
GAMMA = 0.9
KW = dict(alpha=1.0, decay=0.01 ** (1.0 / max(T, 1)), explor=0.2, q_init=1.0)         # Littman's settings


def quartiles(x):
    return "min %.4f  q1 %.4f  median %.4f  q3 %.4f  max %.4f" % tuple(np.percentile(x, [0, 25, 50, 75, 100]))


for name, opponent in (("MR", "uniform"), ("MM", "self")):
    env = VectorSoccerEnv(N, width=5, height=4, slip_prob=0.0, seed=SEED, autoreset=True)
    vstar = planners.minimax_value_iteration(env, 1e-10, GAMMA)[2]
    env.reset()
    pop = env.minimax_q_population(GAMMA, opponent=opponent, **KW)
    pop.run(T)
    worst = np.zeros(N)
    for c0 in range(0, N, 256):                     # a range of members at a time: whole populations run to gigabytes
        worst[c0:c0 + 256] = np.abs(pop.read(c0, min(256, N - c0))["V"] - vstar)[:, 1:].max(1)
    gap = (vstar - pop.exploitability(theta=1e-8)["v_a"])[:, 1:].mean(1)
    print("%s: %d learners x %d steps, training episodes (-1, 0, +1) %s" % (name, N, T, env.episode_histogram().tolist()))
    print("  max |V - V*|     " + quartiles(worst))
    print("  gap of pi_a      " + quartiles(gap))
    pop.close(); env.close()
