"""Gradient play with exact policy gradients (SoccerBatch.gradient_play, planners.policy_gradient): nothing is sampled.
1. Self-play from the uniform pair on 5x4 without slip: four learners, the plain gradient D * Q (step 8) against the gradient
   normalised by the occupancy (step 1), each with optimism 0 and 1.  Every ten steps the exact kick-off exploitability of the
   current pair is printed (planners.exploitability: the value of the best response to pi_b minus that of the best response to
   pi_a, averaged over the initial states).
2. A challenger against a league: a short PSRO run (planners.psro) gives player B's set and its meta-game mixture y; one policy
   of player A is refined by gradient ascent on sum_j y[j] * payoff(x, pi_b[j]) — the exact gradient against a kick-off
   mixture, which no single Markov opponent reproduces — with player B's step at 0, and scored with cross_play against each
   member before and after.
Prints tables; asserts nothing.

    python examples/gradient_play.py [steps] [psro iterations] [psro steps] [lanes]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_soccer_littman94_amd import VectorSoccerEnv  # noqa: E402
from gym_soccer_littman94_amd import planners as pl  # noqa: E402

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 40
ITER = int(sys.argv[2]) if len(sys.argv) > 2 else 4
T = int(sys.argv[3]) if len(sys.argv) > 3 else 5000
N = int(sys.argv[4]) if len(sys.argv) > 4 else 256
GAMMA, THETA = 0.9, 1e-10

env = VectorSoccerEnv(N, width=5, height=4, slip_prob=0.0, seed=1994, autoreset=True)
obs0, _ = env.reset()
starts = np.unique(obs0["player_a"])                # the initial states

# ---- 1. self-play from the uniform pair ---------------------------------------------------------------------------------------
kinds = [("plain, eta 8", dict(normalize=False, eta_a=8.0, eta_b=8.0)), ("normalised, eta 1", dict(normalize=True, eta_a=1.0, eta_b=1.0))]
learners = [("%s, optimism %d" % (name, opt), env.gradient_play(discount_factor=GAMMA, theta=THETA, optimism=float(opt), **kw))
            for name, kw in kinds for opt in (0, 1)]
print("exact kick-off exploitability of the pair, self-play from the uniform pair (5x4, no slip, gamma %.1f)" % GAMMA)
print("step  " + "  ".join("%-28s" % name for name, _ in learners))
for step in range(0, STEPS + 1, 10):
    gaps = [g.exploitability(THETA)["gap"][0, starts].mean() for _, g in learners]
    print("%4d  " % step + "  ".join("%-28.5f" % x for x in gaps))
    for _, g in learners:
        g.run(min(10, STEPS - step))
for _, g in learners:
    g.close()

# ---- 2. a challenger refined against a fixed league mixture -------------------------------------------------------------------------
r = pl.psro(env, ITER, T, GAMMA, theta=1e-8, explor=0.2)
league, y = r["pi_b"], np.asarray(r["y"][-1], np.float64)
y = np.concatenate([y, np.zeros(len(league) - len(y))])               # (a policy added in the last iteration has no weight yet)
print("\nplayer B's league after %d PSRO iterations: %d policies, meta-game weights %s" % (ITER, len(league), np.round(y, 3).tolist()))
g = env.gradient_play(n_a=1, n_b=len(league), discount_factor=GAMMA, theta=THETA, eta_a=1.0, eta_b=0.0, normalize=True, pi_b=league)
g.weights(w_b=y)
before = g.cross_play()["payoff"][0]
trace = g.run(STEPS, trace=True)
after = g.cross_play()["payoff"][0]
print("the challenger (uniform at first) against each member, player A's value at kick-off")
print("member   weight     before      after %d steps" % STEPS)
for j in range(len(league)):
    print("%6d  %7.3f  %+.5f  %+.5f" % (j, y[j], before[j], after[j]))
print("against the mixture: %+.5f -> %+.5f (by step: %s)" % (before @ y, after @ y, np.round(trace[::10, 0] @ y, 4).tolist()))
g.close()
env.close()
