"""The independent Q-learners on the device (SoccerBatch.q_learning): wall time per learner step of run(1000), beside the two
existing paths it is measured against on the same handle, the same way — one minimax-Q learner step (run(1000) of
SoccerBatch.minimax_q) and one step of the mixed-policy rollout — and step 0 (right after a reset every lane sits on an ISD
state: the atomics' worst case) against a steady-state step; QQ (both players epsilon-greedy) and QR (a uniform B), on 5x4
and 11x7 at slip 0 and 0.2 with 2^16 and 2^20 lanes.  With --learn also the wall time of the learning run of
tests/test_gpu_q_learning.py (65 536 lanes x 3 000 steps).  Medians of --repeats runs after a warm-up.  Device times per
kernel come from running this tool under a kernel trace; counters never in the same run.

    python tools/q_learning_time.py [--json OUT] [--learn] [--quick]
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
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def learner_times(b, q, steps, repeats):
    """(step 0, one steady-state step, per step of run(steps): median, min, max) in seconds"""
    b.reset()
    t0s = []
    for _ in range(repeats + 1):                                # step 0: every lane on an ISD state (a reset before each)
        b.reset(); t0s.append(wall(b, lambda: q.run(1), 1)[0])
    q.run(200)                                                  # warm-up: the lanes spread over the pitch
    t_one = wall(b, lambda: q.run(1), repeats)[0]               # launch latency included
    t_run = [x / steps for x in wall(b, lambda: q.run(steps), repeats)]
    return float(np.median(t0s[1:])), t_one, t_run


def run(w, h, slip, n, steps, repeats):
    b = SoccerBatch(n, w, h, slip, seed=1994, autoreset=True)
    kw = dict(decay=0.999, explor=0.2, q_init=0.0)
    out = {"pitch": "%dx%d" % (w, h), "slip": slip, "lanes": n, "n_states": b.nS, "steps": steps, "repeats": repeats}
    for name, acts in (("qq", dict(act_a="greedy", act_b="greedy")), ("qr", dict(act_a="greedy", act_b="uniform"))):
        q = b.q_learning(GAMMA, **acts, **kw)
        s0, one, (med, lo, hi) = learner_times(b, q, steps, repeats)
        out.update({name + "_step0_us": s0 * 1e6, name + "_single_step_us": one * 1e6, name + "_run_step_us": med * 1e6,
                    name + "_run_step_min_us": lo * 1e6, name + "_run_step_max_us": hi * 1e6})
        pi_a = q.read()["pi_a"]
        q.close()
    # the yardsticks: the same handle's minimax-Q step and its mixed-policy rollout, one step per launch
    mq = b.minimax_q(GAMMA, **kw)
    s0, one, (med, lo, hi) = learner_times(b, mq, steps, repeats)
    out.update({"minimax_q_step0_us": s0 * 1e6, "minimax_q_single_step_us": one * 1e6, "minimax_q_run_step_us": med * 1e6,
                "minimax_q_run_step_min_us": lo * 1e6, "minimax_q_run_step_max_us": hi * 1e6})
    mq.close()
    mix = b.alloc((b.nS, 4), np.uint16).upload(SoccerBatch.mixed_policy_thresholds(0.8 * pi_a + 0.04))
    med, lo, hi = [x / steps for x in wall(b, lambda: [b.rollout(1, sample_actions=True, mix_a=mix) for _ in range(steps)], repeats)]
    out.update({"rollout_step_us": med * 1e6, "rollout_step_min_us": lo * 1e6, "rollout_step_max_us": hi * 1e6,
                "qq_over_minimax_q": out["qq_run_step_us"] / out["minimax_q_run_step_us"],
                "qq_over_rollout": out["qq_run_step_us"] / (med * 1e6)})
    b.close()
    return out


def learn():
    n, T = 65536, 3000
    b = SoccerBatch(n, 5, 4, 0.0, seed=1994, autoreset=True)
    want = b.best_response(np.full((b.nS, 5), 0.2), 1, 1e-10, GAMMA)[1]
    q = b.q_learning(GAMMA, alpha=1.0, decay=0.01 ** (1.0 / T), explor=0.2, q_init=0.0, act_b="uniform")
    b.reset(); b.sync()
    t0 = time.perf_counter(); q.run(T); r = q.read(); t = time.perf_counter() - t0
    err = np.abs(r["V_a"] - want)[1:]
    out = {"lanes": n, "steps": T, "device_s": t, "mean_err": float(err.mean()), "max_err": float(err.max())}
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
