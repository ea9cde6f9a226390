"""Minimax-Q (Littman 1994) on the device: train on 65 536 lanes, then let the learned strategy of player A play a
uniformly random player B and print the episode histogram.

    python examples/minimax_q.py [steps]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_soccer_littman94_amd import VectorSoccerEnv, planners  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
env = VectorSoccerEnv(65536, width=5, height=4, slip_prob=0.0, seed=1994, autoreset=True)
env.reset()
pi_a, pi_b, V, Q, visits = planners.minimax_q_learning(env, T, 0.9, explor=0.2, q_init=0.0)
print("trained %d steps x %d lanes; states visited %d / %d; training episodes (-1, 0, +1) %s"
      % (T, env.num_envs, int((visits.sum(1) > 0).sum()), env.nS - 1, env.episode_histogram().tolist()))
v_star = planners.minimax_value_iteration(env, 1e-10, 0.9)[2]
print("max |V - V*| over the live states: %.4f" % np.abs(V - v_star)[1:].max())
env.batch.reset_stats()
env.rollout(100, sample_actions=True, mixed_policies={"player_a": pi_a}, infos="none")
print("learned pi_A against a uniform B, 100 steps: episodes (-1, 0, +1) %s" % env.episode_histogram().tolist())
env.close()
