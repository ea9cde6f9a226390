"""Where the game is played, exactly (planners.occupancy): minimax-Q trained against a uniformly random opponent (MR) and
ordinary Q-learning trained against itself (QQ), as in examples/match_table.py, each pi_A against the uniform opponent and
against its own exact best response.  Per pairing: how long a game lasts when every step has a 0.1 chance of ending it, the
share of those steps in which A has the ball, the mean column of the ball, and the ten most visited states — numbers a sampled
rollout gives only with noise and a bias towards short games.  Then one PSRO league (planners.psro) collapsed against its
challenger (planners.collapse_mixture): the Markov policy that plays like the kick-off mixture of player A's set, which the
state-wise average of the set's policies does not.  Prints tables; asserts nothing.

    python examples/occupancy.py [steps] [lanes] [psro iterations]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_soccer_littman94_amd import VectorSoccerEnv, planners  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
N = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
ITER = int(sys.argv[3]) if len(sys.argv) > 3 else 4
GAMMA, CONTINUE, THETA = 0.9, 0.9, 1e-10
KW = dict(alpha=1.0, decay=0.01 ** (1.0 / max(T, 1)), explor=0.2, q_init=0.0)
SETUPS = [("MR", "minimax_q", dict(opponent="uniform")), ("QQ", "q_learning", dict(act_a="greedy", act_b="greedy"))]

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
env = VectorSoccerEnv(min(N, 4096), width=5, height=4, slip_prob=0.0, seed=94, autoreset=True)
feats = planners.pitch_features(env)
F = np.stack([feats["possession_a"], feats["ball_col"]])
uniform = np.full((env.nS, 5), 0.2)
br_b = np.eye(5)[planners.exploitability(env, pi_a, uniform, THETA, GAMMA)["br_b"]]      # one-hot, [2, nS, 5]
vs_uniform = planners.occupancy(env, pi_a, uniform, THETA, CONTINUE, features=F, values=True)
vs_best = planners.occupancy(env, pi_a, br_b, THETA, CONTINUE, features=F, values=True)  # the diagonal: each against its own


def square(s):
    return "A(%d,%d) B(%d,%d) %s" % (feats["row_a"][s], feats["col_a"][s], feats["row_b"][s], feats["col_b"][s],
                                     "A" if feats["possession_a"][s] else "B")


print("\n(columns count the goal columns: the pitch is columns 1 .. 5)")
print("policy  opponent       steps a game   A has the ball   mean ball column   sweeps")
for i, k in enumerate(names):
    for who, r, j in (("uniform", vs_uniform, 0), ("best response", vs_best, i)):
        L, e = r["length"][i, j], r["expect"][i, j]
        print("%-6s  %-13s  %12.3f  %13.1f %%  %17.3f  %7d" % (k, who, L, 100 * e[0] / L, e[1] / L, r["iterations"][i, j]))
        share = r["visit_share"][i, j]
        top = np.argsort(-share, kind="stable")[:10]
        print("        the ten most visited states (rows, columns, who has the ball: share of the steps)")
        print("        " + ";  ".join("%s: %.1f %%" % (square(s), 100 * share[s]) for s in top))

# one PSRO league collapsed against its challenger
r = planners.psro(env, ITER, T, GAMMA, theta=1e-8, explor=0.2)
Pa, Pb = r["pi_a"], r["pi_b"]
# the league: the most mixed of the meta-strategies PSRO met on the way (the sets only grow at their ends, so an iteration's
# x weighs the first len(x) policies of the final set); if every one of them was pure, the final set with equal weights
xs = r["x"] + [np.asarray(env.solve_meta_game(r["payoff"])["x"], np.float64)]
x = min(xs, key=lambda v: float(np.max(v)))
how = "a meta-strategy of PSRO"
if x.max() > 0.999:
    x, how = np.full(Pa.shape[0], 1.0 / Pa.shape[0]), "every meta-strategy was pure: equal weights instead"
Pa = Pa[:x.size]
challenger = Pb[-1]
sigma, occ = planners.collapse_mixture(env, Pa, x, 0, challenger, THETA, GAMMA)
mixture = float(np.dot(x, r["payoff"][:x.size, -1]))
average = np.einsum("k,ksa->sa", x, Pa)
scores = planners.cross_play(env, np.stack([sigma, average]), challenger, THETA, GAMMA)["payoff"][:, 0]
print("\nPSRO after %d iterations: %d policies of player A with weights %s (%s) against player B's latest policy" % (
    ITER, Pa.shape[0], np.round(x, 3).tolist(), how))
print("  the kick-off mixture scores          %+.8f" % mixture)
print("  collapsed by occupancy, it scores    %+.8f" % scores[0])
print("  the state-wise average scores        %+.8f" % scores[1])
print("  the mixture's game lasts %.3f discounted steps and reaches %d of %d states" % (occ.sum(), int((occ > 0).sum()), env.nS))
env.close()
