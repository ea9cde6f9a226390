"""Bowling & Veloso (2002)'s experiment on this pitch as a distribution over many trials, a learner per lane
(SoccerBatch.wolf_population): n WoLF-PHC pairs and n PHC pairs train in self-play, every member with its own tables, policies
and Philox stream, and the exact gap of every member's pair — how badly the best possible opponent beats it
(WolfPopulation.exploitability) — is printed as quartiles over the members, for the policies pi and for their averages avg.
Then player A of every WoLF member is frozen (WolfPopulation.challengers: a copy on the device) and a challenger per member
learns against it from scratch; the quartiles of the challengers' shortfall against the exact best response to that member's
frozen policy follow.  Prints tables; asserts nothing.

    python examples/wolf_population.py [steps] [members] [seed]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_soccer_littman94_amd import VectorSoccerEnv  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
N = int(sys.argv[2]) if len(sys.argv) > 2 else 512
SEED = int(sys.argv[3]) if len(sys.argv) > 3 else 1994
GAMMA = 0.9
KW = dict(alpha=1.0, decay=0.01 ** (1.0 / max(T, 1)), explor=0.2, q_init=0.0)
WOLF, PHC = dict(delta_win=0.01, delta_lose=0.04), dict(delta_win=0.04, delta_lose=0.04)


def quartiles(x):
    return "min %.4f  q1 %.4f  median %.4f  q3 %.4f  max %.4f" % tuple(np.percentile(x, [0, 25, 50, 75, 100]))


def self_play(name, deltas):
    env = VectorSoccerEnv(N, width=5, height=4, slip_prob=0.0, seed=SEED, autoreset=True)
    env.reset()
    pop = env.wolf_population(GAMMA, **deltas, **KW)
    pop.run(T)
    gaps = {w: pop.exploitability(w, theta=1e-8)["gap"][:, 1:].mean(1) for w in ("pi", "avg")}   # per member: the mean over the live states
    print("trained %-5s %d pairs x %d steps, training episodes (-1, 0, +1) %s" % (name, N, T, env.episode_histogram().tolist()))
    return env, pop, gaps


env, wolf, wolf_gap = self_play("WoLF", WOLF)
env_phc, phc, phc_gap = self_play("PHC", PHC)
phc.close(); env_phc.close()
print("\nexact gap of a member's pair, mean over the live states; quartiles over the %d members" % N)
for name, gap in (("WoLF", wolf_gap), ("PHC ", phc_gap)):
    for w in ("pi", "avg"):
        print("%s %-3s " % (name, w) + quartiles(gap[w]))

# the challenger protocol: freeze player A of every member, train a challenger B per member against it
b = env._batch
ch = wolf.challengers(0, "pi", **WOLF, **KW)
ch.run(T)
short = np.zeros(N)
for c0 in range(0, N, 256):                         # best_response and evaluate_policies take at most 256 policies
    frozen = wolf.read(c0, min(256, N - c0))["pi_a"]
    mine = ch.read(c0, frozen.shape[0])["pi_b"]
    best = b.best_response(frozen, 0, 1e-8, GAMMA)[1]                # player A's value when B answers exactly
    got = b.evaluate_policies(frozen, mine, 1e-8, GAMMA)[0]          # player A's value against the challenger
    short[c0:c0 + frozen.shape[0]] = (got - best)[:, 1:].mean(1)
print("\nchallengers against the frozen player A of every WoLF member, %d steps: V(frozen, challenger) - V(frozen, exact best "
      "response), mean over the live states; quartiles over the %d members" % (T, N))
print("shortfall " + quartiles(short))
ch.close(); wolf.close(); env.close()
