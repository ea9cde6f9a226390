"""Minimax-Q (Littman 1994) on the device: train on 65 536 lanes, keep the strategy of player A every few hundred steps,
then ask for each of them how badly the best possible opponent beats it — one batched best-response solve — and let the
last one play a uniformly random player B.

    python examples/minimax_q.py [steps] [steps between checkpoints]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_soccer_littman94_amd import VectorSoccerEnv, planners  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
EVERY = int(sys.argv[2]) if len(sys.argv) > 2 else max(T // 10, 1)
GAMMA = 0.9
env = VectorSoccerEnv(65536, width=5, height=4, slip_prob=0.0, seed=1994, autoreset=True)
obs, _ = env.reset()
starts = np.unique(obs["player_a"])
learner = env.minimax_q(GAMMA, alpha=1.0, decay=0.01 ** (1.0 / max(T, 1)), explor=0.2, q_init=0.0)
marks, checkpoints = [0], [learner.pi_a]
while marks[-1] < T:
    n = min(EVERY, T - marks[-1])
    learner.run(n)
    marks.append(marks[-1] + n); checkpoints.append(learner.pi_a)
r = learner.read()
V, visits = r["V"], r["visits"]
print("trained %d steps x %d lanes; states visited %d / %d; training episodes (-1, 0, +1) %s"
      % (T, env.num_envs, int((visits.sum(1) > 0).sum()), env.nS - 1, env.episode_histogram().tolist()))
v_star = planners.minimax_value_iteration(env, 1e-10, GAMMA)[2]
print("max |V - V*| over the live states: %.4f" % np.abs(V - v_star)[1:].max())
# every checkpoint's worst case in one batch: B answers pi_A as well as anyone can
_, v_a, _, sweeps = planners.best_response(env, np.stack(checkpoints), 0, 1e-10, GAMMA)
print("worst case of pi_A (V* at the initial states: %s)" % np.round(v_star[starts], 4).tolist())
for m, v, k in zip(marks, v_a, sweeps):
    print("  after %5d steps: at the initial states %s, V* - worst case over the live states: mean %.4f max %.4f (%d sweeps)"
          % (m, np.round(v[starts], 4).tolist(), (v_star - v)[1:].mean(), (v_star - v)[1:].max(), k))
env.batch.reset_stats()
env.rollout(100, sample_actions=True, mixed_policies={"player_a": r["pi_a"]}, infos="none")
print("learned pi_A against a uniform B, 100 steps: episodes (-1, 0, +1) %s" % env.episode_histogram().tolist())
learner.close()
env.close()
