"""Policy hill-climbing on Littman's pitch (Bowling & Veloso 2002): WoLF-PHC and plain PHC trained in self-play on the device,
a WoLF challenger trained against each frozen policy of the WoLF pair (Littman's challenger protocol), and ordinary
Q-learning in self-play (QQ) beside them.  Every pair of policies is graded exactly — how badly does the best possible
opponent beat it (planners.exploitability) — for the policies and for their running averages.  Prints a table; asserts
nothing, and at this budget claims no ranking: one seed's self-play gaps of the three learners are too close for one
(DESIGN.md §13).  A challenger that wins quickly visits few states; its shortfall is taken over all live states.

    python examples/wolf_phc.py [steps] [lanes] [seed]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_soccer_littman94_amd import SoccerBatch, VectorSoccerEnv, planners  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
N = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
SEED = int(sys.argv[3]) if len(sys.argv) > 3 else 1994
GAMMA = 0.9
KW = dict(alpha=1.0, decay=0.01 ** (1.0 / max(T, 1)), explor=0.2, q_init=0.0)


def train(kind, **how):
    env = VectorSoccerEnv(N, width=5, height=4, slip_prob=0.0, seed=SEED, autoreset=True)
    env.reset()
    learner = getattr(env, kind)(GAMMA, **how, **KW)
    learner.run(T)
    r = learner.read()
    print("trained %-11s %d steps x %d lanes, states visited %d / %d, training episodes (-1, 0, +1) %s"
          % (kind, T, N, int((r["visits"].sum(1) > 0).sum()), env.nS - 1, env.episode_histogram().tolist()))
    learner.close()
    env.close()
    return r


wolf = train("wolf_phc", delta_win=0.01, delta_lose=0.04)
phc = train("wolf_phc", delta_win=0.04, delta_lose=0.04)
qq = train("q_learning", act_a="greedy", act_b="greedy")
# the challengers: a WoLF learner against each frozen policy of the WoLF pair
vs_a = train("wolf_phc", delta_win=0.01, delta_lose=0.04, act_a=wolf["pi_a"], act_b="learn")
vs_b = train("wolf_phc", delta_win=0.01, delta_lose=0.04, act_a="learn", act_b=wolf["pi_b"])

grader = SoccerBatch(64, 5, 4, 0.0, seed=SEED, autoreset=True)     # the exact solves need a handle, not its lanes
pairs = [("WoLF-PHC   pi", wolf["pi_a"], wolf["pi_b"]), ("WoLF-PHC   avg", wolf["avg_a"], wolf["avg_b"]),
         ("PHC        pi", phc["pi_a"], phc["pi_b"]), ("PHC        avg", phc["avg_a"], phc["avg_b"]),
         ("QQ         greedy", qq["pi_a"], qq["pi_b"])]
e = planners.exploitability(grader, np.stack([p[1] for p in pairs]), np.stack([p[2] for p in pairs]), 1e-10, GAMMA)
print("\nself-play pair      exact gap of the pair over the live states (mean, max)")
for i, (name, _, _) in enumerate(pairs):
    gap = e["gap"][i][1:]
    print("%-18s  %.4f  %.4f" % (name, gap.mean(), gap.max()))

# what the challengers found against what was there to find: player A's value of (frozen, challenger) beside the exact
# best response to the frozen policy
V = grader.evaluate_policies(np.stack([wolf["pi_a"], vs_b["pi_a"]]), np.stack([vs_a["pi_b"], wolf["pi_b"]]), 1e-10, GAMMA)[0]
short_b = (V[0] - e["v_a"][0])[1:]          # B challenges the frozen pi_a: it wants player A's value low
short_a = (e["v_b"][0] - V[1])[1:]          # A challenges the frozen pi_b: it wants it high
print("\nchallenger          falls short of the exact best response by (mean, max)")
print("%-18s  %.4f  %.4f" % ("B against pi_a", short_b.mean(), short_b.max()))
print("%-18s  %.4f  %.4f" % ("A against pi_b", short_a.mean(), short_a.max()))
grader.close()
