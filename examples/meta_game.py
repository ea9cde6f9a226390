"""Which mixture of a trained population can a rational opponent not beat, and how much better is it than the best single
member?  n independent Q-learner pairs train in self-play, a learner per lane (SoccerBatch.q_population); every member's
player A then meets every member's player B (the exact n x n cross-play matrix), and the matrix game over the members is
solved on the device (QPopulation.meta_game: maximin mixtures x and y with the bracket lo <= value <= hi they certify).
Prints the support sizes, the mixture's guarantee beside the best single member's worst case in the set (row_min), and the
solver's status.  Prints tables; asserts nothing.

    python examples/meta_game.py [steps] [members] [seed]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_soccer_littman94_amd import VectorSoccerEnv  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
N = int(sys.argv[2]) if len(sys.argv) > 2 else 32
SEED = int(sys.argv[3]) if len(sys.argv) > 3 else 1994
GAMMA, THETA = 0.9, 1e-8
STATUS = {0: "finished, bracket within eps", 1: "pure saddle point", 2: "finished, bracket wider than eps", 3: "stopped at max_pivots"}

env = VectorSoccerEnv(N, width=5, height=4, slip_prob=0.0, seed=SEED, autoreset=True)
env.reset()
pop = env.q_population(GAMMA, alpha=1.0, decay=0.01 ** (1.0 / max(T, 1)), explor=0.2)
pop.run(T)
print("trained %d Q-learner pairs x %d steps, training episodes (-1, 0, +1) %s" % (N, T, env.episode_histogram().tolist()))

m = pop.meta_game(theta=THETA)
best = int(np.argmax(m["row_min"]))
print("\nplayer A's value at kick-off, %d x %d pairs, %d .. %d sweeps a pair" % (N, N, m["iterations"].min(), m["iterations"].max()))
print("best single member (A side)  member %d, worst opponent in the set %+.6f (pure maximin)" % (best, m["bounds"][0]))
print("best single member (B side)  member %d, concedes at most %+.6f (pure minimax)" % (int(np.argmin(m["col_max"])), m["bounds"][1]))
print("maximin mixture of A's       guarantees %+.6f against every B in the set: gain %+.6f" % (m["lo"], m["gain"]))
print("minimax mixture of B's       concedes at most %+.6f" % m["hi"])
print("meta-game value              %+.6f  (hi - lo = %.2e)" % (m["value"], m["hi"] - m["lo"]))
print("support                      %d of %d A policies, %d of %d B policies" % ((m["x"] > 0).sum(), N, (m["y"] > 0).sum(), N))
print("A's mixture                  " + ", ".join("member %d: %.3f" % (i, m["x"][i]) for i in np.flatnonzero(m["x"] > 0)))
print("status                       %d (%s)" % (m["status"], STATUS[int(m["status"])]))
pop.close(); env.close()
