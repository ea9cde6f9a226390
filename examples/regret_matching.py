"""Regret matchers with one table that every lane feeds (SoccerBatch.regret_matching): the shared form of
examples/regret_population.py.  Self-play (both players learn) on 5x4 with 65 536 lanes, once per setting: regret matching+ with
plain averaging, regret matching+ with linear averaging, and plain regret matching.  At a few checkpoints the exact gap — how
badly the best possible opponent beats the pair (RegretLearner.exploitability), mean over the live states — of the AVERAGE
policies (the pair that carries the no-regret guarantee) and of the current policies is printed beside that of a wolf_phc
trained with the same seed for the same steps.  Prints a table; asserts nothing.

    python examples/regret_matching.py [steps] [lanes] [seed]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_soccer_littman94_amd import VectorSoccerEnv  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
N = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
SEED = int(sys.argv[3]) if len(sys.argv) > 3 else 1994
GAMMA = 0.9
KW = dict(alpha=1.0, decay=0.01 ** (1.0 / max(T, 1)), q_init=0.0, explor=0.2)
CHECKPOINTS = sorted({max(T // 8, 1), max(T // 4, 1), max(T // 2, 1), T})


def train(kind, **how):
    """-> [(steps, mean gap of the average pair, of the current pair)] at the checkpoints"""
    env = VectorSoccerEnv(N, width=5, height=4, slip_prob=0.0, seed=SEED, autoreset=True)
    env.reset()
    q = getattr(env, kind)(GAMMA, **how, **KW)
    rows, done = [], 0
    for t in CHECKPOINTS:
        q.run(t - done)
        done = t
        rows.append((t, q.exploitability("avg", theta=1e-8)["gap"][1:].mean(), q.exploitability("pi", theta=1e-8)["gap"][1:].mean()))
    q.close()
    env.close()
    return rows


runs = [("regret matching+", train("regret_matching", plus=True, linear=False)),
        ("regret matching+, linear", train("regret_matching", plus=True, linear=True)),
        ("regret matching", train("regret_matching", plus=False, linear=False)),
        ("WoLF-PHC", train("wolf_phc", delta_win=0.01, delta_lose=0.04))]

print("self-play, 5x4, slip 0, %d lanes, seed %d; exact gap of the pair of policies, mean over the live states" % (N, SEED))
print("%-26s %8s %10s %10s" % ("", "steps", "avg", "pi"))
for name, rows in runs:
    for t, avg, pi in rows:
        print("%-26s %8d %10.4f %10.4f" % (name, t, avg, pi))
