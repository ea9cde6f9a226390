"""The minimax-Q learner on the device (SoccerBatch.minimax_q): wall time per learner step of run(1000), beside the two
things a step is made of, measured the same way on the same handle — one step of the mixed-policy rollout and one
minimax value iteration sweep — and step 0 (right after a reset every lane sits on an ISD state: the atomics' worst case)
against a steady-state step; on 5x4 and 11x7 at slip 0 and 0.2 with 2^16 and 2^20 lanes.  With --learn also the wall time
of the learning run of tests/test_gpu_minimax_q.py (65 536 lanes x 3 000 steps).  Medians of --repeats runs after a
warm-up.  Device times per kernel come from running this tool under a kernel trace; counters never in the same run.

    python tools/minimax_q_time.py [--json OUT] [--learn] [--quick]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_soccer_littman94_amd import SoccerBatch  # noqa: E402

GAMMA = 0.9


def wall(b, fn, repeats):
    ts = []
    for _ in range(repeats):
        b.sync(); t0 = time.perf_counter(); fn(); b.sync(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def run(w, h, slip, n, steps, repeats):
    b = SoccerBatch(n, w, h, slip, seed=1994, autoreset=True)
    q = b.minimax_q(GAMMA, decay=0.999, explor=0.2, q_init=0.0)
    b.reset()
    # step 0: every lane on an ISD state (a reset before each)
    t0s = []
    for _ in range(repeats + 1):
        b.reset(); t0s.append(wall(b, lambda: q.run(1), 1))
    q.run(200)                                                  # warm-up: the lanes spread over the pitch
    t_one = wall(b, lambda: q.run(1), repeats)                  # one steady-state step, launch latency included
    t_run = wall(b, lambda: q.run(steps), repeats) / steps
    # the yardstick: the same handle's mixed-policy rollout, one step per launch, and one Shapley sweep
    mix = b.alloc((b.nS, 4), np.uint16).upload(SoccerBatch.mixed_policy_thresholds(0.8 * q.pi_a + 0.04))
    t_roll = wall(b, lambda: [b.rollout(1, sample_actions=True, mix_a=mix) for _ in range(steps)], repeats) / steps
    V = np.zeros(b.nS)
    b.minimax_backup(V, GAMMA)                                  # builds the lists
    t0 = time.perf_counter(); k = b.minimax_value_iteration(1e-10, GAMMA)[4]; t_sweep = (time.perf_counter() - t0) / k
    out = {"pitch": "%dx%d" % (w, h), "slip": slip, "lanes": n, "n_states": b.nS,
           "step0_us": float(np.median(t0s[1:])) * 1e6, "single_step_us": t_one * 1e6, "run_step_us": t_run * 1e6,
           "rollout_step_us": t_roll * 1e6, "sweep_us": t_sweep * 1e6, "yardstick_us": (t_roll + t_sweep) * 1e6,
           "ratio": t_run / (t_roll + t_sweep)}
    b.close()
    return out


def learn():
    n, T = 65536, 3000
    b = SoccerBatch(n, 5, 4, 0.0, seed=1994, autoreset=True)
    vstar = b.minimax_value_iteration(1e-10, GAMMA)[2]
    q = b.minimax_q(GAMMA, alpha=1.0, decay=0.01 ** (1.0 / T), explor=0.2, q_init=0.0)
    b.reset(); b.sync()
    t0 = time.perf_counter(); q.run(T); r = q.read(); t = time.perf_counter() - t0
    out = {"lanes": n, "steps": T, "device_s": t, "max_err": float(np.abs(r["V"] - vstar)[1:].max())}
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json"); ap.add_argument("--learn", action="store_true"); ap.add_argument("--quick", action="store_true")
    ap.add_argument("--steps", type=int, default=1000); ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    cases = [(5, 4, 0.0), (5, 4, 0.2), (11, 7, 0.0), (11, 7, 0.2)]
    lanes = [1 << 16, 1 << 20]
    if a.quick:
        cases, lanes = cases[:1], lanes[:1]
    rows = []
    for w, h, slip in cases:
        for n in lanes:
            rows.append(run(w, h, slip, n, a.steps, a.repeats))
            print(json.dumps(rows[-1]), flush=True)
    out = {"rows": rows}
    if a.learn:
        out["learn"] = learn()
        print(json.dumps(out["learn"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
