"""The regret matchers of one table on the device (SoccerBatch.regret_matching): warm wall time per learner step of run(steps)
with both players LEARN (regret matching+, plain averaging), and on the same handle, measured the same way, its nearest
neighbour: a step of the policy hill-climbers (SoccerBatch.wolf_phc), whose act and reduce are the same code and whose update
kernel has the same shape.  5x4, slip 0 and 0.2, 2^16 and 2^20 lanes.  The two are ALTERNATED repeat by repeat so that a drift
of the machine falls on both; median, minimum and maximum of --repeats runs after one warm-up call each, and the ratio of the
medians with the ratios of the single repeats' extremes.  wolf_phc is the yardstick; there is no pass mark.

    python tools/regret_matching_time.py [--json OUT] [--quick] [--steps 2000] [--repeats 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GAMMA = 0.9
CASES = [(5, 4, slip, n) for slip in (0.0, 0.2) for n in (1 << 16, 1 << 20)]
KW = dict(decay=0.9999, explor=0.2, q_init=0.0)


def timed(b, fn):
    b.sync(); t0 = time.perf_counter(); fn(); b.sync()
    return time.perf_counter() - t0


def run(w, h, slip, n, steps, repeats):
    from gym_soccer_littman94_amd import SoccerBatch
    b = SoccerBatch(n, w, h, slip, seed=1994, autoreset=True)
    out = {"pitch": "%dx%d" % (w, h), "slip": slip, "lanes": n, "n_states": b.nS, "steps": steps, "repeats": repeats}
    regret = b.regret_matching(GAMMA, **KW); wolf = b.wolf_phc(GAMMA, **KW)
    calls = {"regret": lambda: regret.run(steps), "wolf_phc": lambda: wolf.run(steps)}
    b.reset()
    for fn in calls.values():                                   # warm-up: the lanes spread over the pitch, the code is resident
        timed(b, fn)
    ts = {k: [] for k in calls}
    for _ in range(repeats):
        for k, fn in calls.items():                             # alternated
            ts[k].append(timed(b, fn) / steps * 1e6)
    for k, v in ts.items():
        out.update({k + "_step_us": float(np.median(v)), k + "_step_min_us": float(np.min(v)), k + "_step_max_us": float(np.max(v)),
                    k + "_lane_steps_per_s": float(n / (np.median(v) * 1e-6))})
    ratios = np.array(ts["regret"]) / np.array(ts["wolf_phc"])              # repeat by repeat: the pair ran back to back
    out.update({"ratio_regret_over_wolf": float(np.median(ts["regret"]) / np.median(ts["wolf_phc"])),
                "ratio_min": float(ratios.min()), "ratio_max": float(ratios.max())})
    out["misuse"] = int(b.misuse())
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json"); ap.add_argument("--quick", action="store_true")
    ap.add_argument("--steps", type=int, default=2000); ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    rows = []
    for w, h, slip, n in (CASES[:1] if a.quick else CASES):
        rows.append(run(w, h, slip, n, a.steps, a.repeats))
        print(json.dumps(rows[-1]), flush=True)
        if a.json:                                              # after every case: a run cut short keeps what it measured
            with open(a.json, "w") as f:
                json.dump({"rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
