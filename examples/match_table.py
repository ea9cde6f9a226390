"""Littman (1994)'s table for his four learners, exactly: minimax-Q and ordinary Q-learning, each trained against a uniformly
random opponent (MR, QR) and against itself (MM, QQ) as in examples/littman_table.py, then each pi_A graded against the
uniform opponent and against its own exact best response (planners.exploitability's br_b) in his columns — % won by A, % won
by B, % drawn and games completed in 100 000 steps — when every step has a 0.1 chance of ending the game as a draw
(planners.match_outcomes, continue_prob = 0.9).  The episode histogram of a sampled rollout of the same pair stands beside
them for the eye: its games end at the environment's step limit, not by that chance.  Prints a table; asserts nothing.

    python examples/match_table.py [steps] [lanes]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_soccer_littman94_amd import VectorSoccerEnv, planners  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
N = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
GAMMA, CONTINUE, THETA = 0.9, 0.9, 1e-10
KW = dict(alpha=1.0, decay=0.01 ** (1.0 / max(T, 1)), explor=0.2, q_init=0.0)
SETUPS = [("MR", "minimax_q", dict(opponent="uniform")), ("MM", "minimax_q", dict(opponent="self")),
          ("QR", "q_learning", dict(act_a="greedy", act_b="uniform")), ("QQ", "q_learning", dict(act_a="greedy", act_b="greedy"))]

policies = {}
for name, kind, how in SETUPS:
    env = VectorSoccerEnv(N, width=5, height=4, slip_prob=0.0, seed=1994, autoreset=True)
    env.reset()
    learner = getattr(env, kind)(GAMMA, **how, **KW)
    learner.run(T)
    policies[name] = learner.read()["pi_a"]
    print("%s: trained %d steps x %d lanes" % (name, T, N))
    learner.close()
    env.close()

names = [s[0] for s in SETUPS]
pi_a = np.stack([policies[k] for k in names])
env = VectorSoccerEnv(N, width=5, height=4, slip_prob=0.0, seed=94, autoreset=True)
uniform = np.full((env.nS, 5), 0.2)
br_b = np.eye(5)[planners.exploitability(env, pi_a, uniform, THETA, GAMMA)["br_b"]]      # one-hot, [4, nS, 5]
vs_uniform = planners.match_outcomes(env, pi_a, uniform, THETA, CONTINUE)
vs_best = planners.match_outcomes(env, pi_a, br_b, THETA, CONTINUE)                      # the diagonal: each against its own

print("\npolicy  opponent       % won by A   % won by B   % drawn  games in 100 000 steps   sampled episodes (-1, 0, +1)")
for i, k in enumerate(names):
    for who, r, j, pi_b in (("uniform", vs_uniform, 0, uniform), ("best response", vs_best, i, br_b[i])):
        env.reset()
        before = env.episode_histogram()
        env.rollout(200, sample_actions=True, mixed_policies={"player_a": pi_a[i], "player_b": pi_b})
        print("%-6s  %-13s  %10.2f  %10.2f  %7.2f  %22.0f   %s" % (
            k, who, 100 * r["win_a"][i, j], 100 * r["win_b"][i, j], 100 * r["draw"][i, j], 1e5 * r["games_per_step"][i, j],
            (env.episode_histogram() - before).tolist()))
print("(exact: every step is followed by a 0.1 chance of a draw; sampled: 200 steps x %d lanes, games end at the step limit)" % N)
env.close()
