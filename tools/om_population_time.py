"""The population of opponent-modelling Q-learners (SoccerBatch.om_population, om_pop_run_kernel): member steps per second of
run(steps), and on the same handle, at the same n and steps, measured the same way, the yardstick: the population of
independent Q-learners (q_population, pop_run_kernel).  Both (greedy, greedy).  A step of om_pop_run_kernel moves about 0.5 KB
per member (two 256-byte rows at s, two 16-byte pairs at s') against pop_run_kernel's 80 B, so a ratio well below 1 is
expected; no ratio is fixed in advance.  The two are ALTERNATED repeat by repeat so that a drift of the machine falls on both;
one warm-up each, then median, minimum and maximum of --repeats runs, and the ratio of each repeat's pair.

    python tools/om_population_time.py [--json profiles/om_population_time.json] [--quick] [--steps 10000] [--repeats 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GAMMA = 0.9
CASES = [(5, 4, slip, n) for slip in (0.0, 0.2) for n in (1 << 10, 1 << 14)]
KW = dict(decay=0.9999, explor=0.2, q_init=0.0)


def timed(b, fn):
    b.sync(); t0 = time.perf_counter(); fn(); b.sync()
    return time.perf_counter() - t0


def run(w, h, slip, n, steps, repeats):
    from gym_soccer_littman94_amd import SoccerBatch
    b = SoccerBatch(n, w, h, slip, seed=1994, autoreset=True)
    out = {"pitch": "%dx%d" % (w, h), "slip": slip, "members": n, "n_states": b.nS, "steps": steps, "repeats": repeats,
           "om_table_bytes": n * b.nS * 512, "q_table_bytes": n * b.nS * 80}
    pops = {"q": b.q_population(GAMMA, **KW), "om": b.om_population(GAMMA, **KW)}
    calls = {k: (lambda q=q: q.run(steps)) for k, q in pops.items()}
    b.reset()
    for fn in calls.values():                                   # warm-up: the lanes spread over the pitch, the code is resident
        timed(b, fn)
    ts = {k: [] for k in calls}
    for _ in range(repeats):
        for k, fn in calls.items():                             # alternated
            ts[k].append(n * steps / timed(b, fn))
    for k, v in ts.items():
        out.update({k + "_steps_per_s": float(np.median(v)), k + "_steps_per_s_min": float(np.min(v)), k + "_steps_per_s_max": float(np.max(v))})
    ratio = np.array(ts["om"]) / np.array(ts["q"])              # repeat by repeat: the pair ran back to back
    out.update({"om_over_q": out["om_steps_per_s"] / out["q_steps_per_s"], "om_over_q_min": float(ratio.min()), "om_over_q_max": float(ratio.max())})
    out["misuse"] = int(b.misuse())
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json"); ap.add_argument("--quick", action="store_true")
    ap.add_argument("--steps", type=int, default=10000); ap.add_argument("--repeats", type=int, default=5)
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
