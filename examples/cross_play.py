"""Have self-play partners co-adapted?  n WoLF-PHC pairs train in self-play, a learner per lane (SoccerBatch.wolf_population),
and then every member's player A meets every member's player B (WolfPopulation.cross_play: the exact n x n payoff matrix,
player A's value at kick-off).  Printed as quartiles: the diagonal (each member against the partner it trained with), the
off-diagonal entries (against strangers), and each member's worst opponent in the population (row_min) next to its exact
worst case against any opponent at all (WolfPopulation.exploitability).  Prints tables; asserts nothing.

    python examples/cross_play.py [steps] [members] [seed]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_soccer_littman94_amd import VectorSoccerEnv  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
N = int(sys.argv[2]) if len(sys.argv) > 2 else 64
SEED = int(sys.argv[3]) if len(sys.argv) > 3 else 1994
GAMMA, THETA = 0.9, 1e-8


def quartiles(x):
    return "min %+.4f  q1 %+.4f  median %+.4f  q3 %+.4f  max %+.4f" % tuple(np.percentile(x, [0, 25, 50, 75, 100]))


env = VectorSoccerEnv(N, width=5, height=4, slip_prob=0.0, seed=SEED, autoreset=True)
obs0, _ = env.reset()
starts = np.unique(obs0["player_a"])                # the initial states (with 64 lanes all of them show up)
pop = env.wolf_population(GAMMA, alpha=1.0, decay=0.01 ** (1.0 / max(T, 1)), explor=0.2, q_init=0.0, delta_win=0.01, delta_lose=0.04)
pop.run(T)
print("trained %d WoLF-PHC pairs x %d steps, training episodes (-1, 0, +1) %s" % (N, T, env.episode_histogram().tolist()))

payoff, sweeps = pop.cross_play("pi", theta=THETA)
off = payoff[~np.eye(N, dtype=bool)]
worst = pop.exploitability("pi", theta=THETA)["v_a"][:, starts].mean(1)       # against the exact best response, at kick-off
print("\nplayer A's value at kick-off, %d x %d pairs, %d .. %d sweeps a pair; quartiles" % (N, N, sweeps.min(), sweeps.max()))
print("own partner (diagonal)       " + quartiles(np.diag(payoff)))
print("strangers (off-diagonal)     " + quartiles(off))
print("worst opponent in the set    " + quartiles(payoff.min(1)))
print("exact worst case             " + quartiles(worst))
print("worst in the set - exact     " + quartiles(payoff.min(1) - worst))
print("pure maximin %.4f <= meta-game value <= pure minimax %.4f" % (payoff.min(1).max(), payoff.max(0).min()))
pop.close(); env.close()
