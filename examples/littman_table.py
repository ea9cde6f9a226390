"""Littman (1994)'s four learners with one budget on the device: minimax-Q and ordinary Q-learning, each trained against a
uniformly random opponent (MR, QR) and against itself (MM, QQ), then every resulting pair of policies graded exactly — how
badly does the best possible opponent beat it (planners.exploitability)?  Prints a table; asserts nothing.

    python examples/littman_table.py [steps] [lanes]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_soccer_littman94_amd import VectorSoccerEnv, planners  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
N = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
GAMMA = 0.9
KW = dict(alpha=1.0, decay=0.01 ** (1.0 / max(T, 1)), explor=0.2, q_init=0.0)
SETUPS = [("MR", "minimax_q", dict(opponent="uniform")), ("MM", "minimax_q", dict(opponent="self")),
          ("QR", "q_learning", dict(act_a="greedy", act_b="uniform")), ("QQ", "q_learning", dict(act_a="greedy", act_b="greedy"))]

policies = {}
for name, kind, how in SETUPS:
    env = VectorSoccerEnv(N, width=5, height=4, slip_prob=0.0, seed=1994, autoreset=True)
    env.reset()
    learner = getattr(env, kind)(GAMMA, **how, **KW)
    learner.run(T)
    r = learner.read()
    policies[name] = (r["pi_a"], r["pi_b"])
    print("%s: trained %d steps x %d lanes, states visited %d / %d, training episodes (-1, 0, +1) %s"
          % (name, T, N, int((r["visits"].sum(1) > 0).sum()), env.nS - 1, env.episode_histogram().tolist()))
    learner.close()
    if name != SETUPS[-1][0]:
        env.close()

v_star = planners.minimax_value_iteration(env, 1e-10, GAMMA)[2]
starts = np.unique(env.reset()[0]["player_a"])
names = [s[0] for s in SETUPS]
e = planners.exploitability(env, np.stack([policies[k][0] for k in names]), np.stack([policies[k][1] for k in names]), 1e-10, GAMMA)
print("\nV* at the initial states: %s" % np.round(v_star[starts], 4).tolist())
print("policy  worst case of pi_A at the initial states   V* - worst case (mean, max)   gap of the pair (mean, max)")
for i, k in enumerate(names):
    loss = (v_star - e["v_a"][i])[1:]
    gap = e["gap"][i][1:]
    print("%-6s  %-43s  %.4f  %.4f               %.4f  %.4f"
          % (k, np.round(e["v_a"][i][starts], 4).tolist(), loss.mean(), loss.max(), gap.mean(), gap.max()))
print("(for MR and QR only pi_A was trained to play: their pi_B is a by-product of learning against a random B)")
env.close()
