"""Policy-space response oracles on the device (planners.psro): from the uniform policy on both sides, every iteration solves
the meta-game of the two policy sets, trains a population of Q-learners against each side's equilibrium MIXTURE — a league
opponent that draws one of the set's policies at every kick-off (SoccerBatch.q_population(act_b="league", ...)) — scores every
learner exactly, and adds the best one to its side's set if it beats the mixture.  Printed per iteration: the set sizes, the
meta-game's bracket lo <= value <= hi, the challengers' best scores and gap = br_a - br_b (a LOWER estimate of the mixture
pair's NashConv: the challengers are learners, not exact best responses), and beside lo / hi the exact exploitability of the
best single member of each side (planners.exploitability at kick-off).  Prints tables; asserts nothing.

    python examples/psro.py [iterations] [steps] [lanes] [seed]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_soccer_littman94_amd import VectorSoccerEnv  # noqa: E402
from gym_soccer_littman94_amd import planners as pl  # noqa: E402

ITER = int(sys.argv[1]) if len(sys.argv) > 1 else 8
T = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
N = int(sys.argv[3]) if len(sys.argv) > 3 else 256
SEED = int(sys.argv[4]) if len(sys.argv) > 4 else 1994
GAMMA, THETA = 0.9, 1e-8

env = VectorSoccerEnv(N, width=5, height=4, slip_prob=0.0, seed=SEED, autoreset=True)
obs0, _ = env.reset()
starts = np.unique(obs0["player_a"])                # the initial states
r = pl.psro(env, ITER, T, GAMMA, theta=THETA, explor=0.2)

# the sets only grow at their ends, so iteration k saw the first |Pi_A|, |Pi_B| policies of the final sets
e = pl.exploitability(env, r["pi_a"], r["pi_b"], THETA, GAMMA)
worst_a = e["v_a"][:, starts].mean(1)               # each A policy against its exact best response, at kick-off
worst_b = e["v_b"][:, starts].mean(1)
print("%d lanes x %d steps a challenger run, %d iterations; player A's value at kick-off" % (N, T, ITER))
print("iter  |Pi_A| |Pi_B|        lo        hi      br_a      br_b       gap   best single A / its exact worst case   best single B / its exact worst case")
sa = sb = 1
for k in range(ITER):
    P = r["payoff"][:sa, :sb]
    ia, ib = int(np.argmax(P.min(1))), int(np.argmin(P.max(0)))
    print("%4d  %6d %6d  %+.5f  %+.5f  %+.5f  %+.5f  %+.5f   A[%d] in the set %+.5f, exactly %+.5f       B[%d] in the set %+.5f, exactly %+.5f"
          % (k, sa, sb, r["lo"][k], r["hi"][k], r["br_a"][k], r["br_b"][k], r["gap"][k], ia, P.min(1)[ia], worst_a[ia], ib, P.max(0)[ib],
             worst_b[ib]))
    sa += int(r["added_a"][k]); sb += int(r["added_b"][k])
print("final sets: %d A policies, %d B policies; sweeps a pair %d .. %d" % (sa, sb, r["iterations"].min(), r["iterations"].max()))
env.close()
