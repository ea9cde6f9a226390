"""A league opponent in the population of Q-learners (SoccerBatch.q_population(act_b="league", ...), pop_league_run_kernel):
member steps per second of run(steps) at K = 1, 16 and 1024 league policies, and on the same handle, at the same n and
steps, measured the same way, the yardstick: the population against ONE shared fixed policy (pop_run_kernel, the kernel that
was there before).  The league adds a pick load and store per launch, a row address that depends on the pick, and a rare
draw; no ratio is fixed in advance.  The four are ALTERNATED repeat by repeat so that a drift of the machine falls on all;
one warm-up each, then median, minimum and maximum of --repeats runs.

    python tools/league_time.py [--json profiles/league_time.json] [--quick] [--steps 10000] [--repeats 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GAMMA = 0.9
KS = (1, 16, 1024)
CASES = [(w, h, slip, n) for (w, h) in ((5, 4),) for slip in (0.0, 0.2) for n in (1 << 10, 1 << 14, 1 << 16)]
KW = dict(decay=0.9999, explor=0.2, q_init=0.0)


def timed(b, fn):
    b.sync(); t0 = time.perf_counter(); fn(); b.sync()
    return time.perf_counter() - t0


def run(w, h, slip, n, steps, repeats):
    from gym_soccer_littman94_amd import SoccerBatch
    b = SoccerBatch(n, w, h, slip, seed=1994, autoreset=True)
    out = {"pitch": "%dx%d" % (w, h), "slip": slip, "members": n, "n_states": b.nS, "steps": steps, "repeats": repeats,
           "table_bytes": n * b.nS * 80}
    rng = np.random.default_rng(11)
    pols = rng.dirichlet(np.ones(5), (max(KS), b.nS))
    pops = {"fixed": b.q_population(GAMMA, act_b=pols[0], **KW)}
    for K in KS:
        wts = rng.dirichlet(np.ones(K))
        pops["league_K%d" % K] = b.q_population(GAMMA, act_b="league", league_policies=pols[:K], league_weights=wts, **KW)
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
    for K in KS:
        out["league_K%d_over_fixed" % K] = out["league_K%d_steps_per_s" % K] / out["fixed_steps_per_s"]
    out["fixed_spread"] = out["fixed_steps_per_s_min"] / out["fixed_steps_per_s"], out["fixed_steps_per_s_max"] / out["fixed_steps_per_s"]
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
