"""The policy hill-climbers on the device (SoccerBatch.wolf_phc): warm wall time per learner step of run(steps), beside the
independent Q-learners (SoccerBatch.q_learning, QQ) on the same handle, the two ALTERNATED repeat by repeat so that a drift
of the machine falls on both; 5x4 at slip 0 and 0.2 and 11x7 at slip 0.2 with 2^16 and 2^20 lanes.  Medians of --repeats
runs after a warm-up, with the spread.

Device times per kernel come from a kernel trace of a run of its own (never in the same run as the wall times, never with
counters): --trace-case I runs case I alone, --repeats times run(steps) of each learner after the warm-up, and nothing else;
--summarise reads the kernel-trace CSVs of such runs and prints the per-kernel medians over all dispatches.

    python tools/wolf_phc_time.py [--json OUT] [--quick]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o case0 -- python tools/wolf_phc_time.py --trace-case 0
    python tools/wolf_phc_time.py --summarise DIR [--json OUT]
"""
import argparse
import csv
import glob
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GAMMA = 0.9
CASES = [(w, h, slip, n) for (w, h, slip) in ((5, 4, 0.0), (5, 4, 0.2), (11, 7, 0.2)) for n in (1 << 16, 1 << 20)]
KW = dict(decay=0.999, explor=0.2, q_init=0.0)


def learners(b):
    return {"wolf_phc": b.wolf_phc(GAMMA, delta_win=0.01, delta_lose=0.04, **KW), "qq": b.q_learning(GAMMA, **KW)}


def timed(b, fn):
    b.sync(); t0 = time.perf_counter(); fn(); b.sync()
    return time.perf_counter() - t0


def run(w, h, slip, n, steps, repeats):
    from gym_soccer_littman94_amd import SoccerBatch
    b = SoccerBatch(n, w, h, slip, seed=1994, autoreset=True)
    qs = learners(b)
    b.reset()
    for q in qs.values():
        q.run(200)                                              # warm-up: the lanes spread over the pitch
    ts = {k: [] for k in qs}
    for _ in range(repeats):
        for k, q in qs.items():                                 # alternated
            ts[k].append(timed(b, lambda: q.run(steps)) / steps * 1e6)
    out = {"pitch": "%dx%d" % (w, h), "slip": slip, "lanes": n, "n_states": b.nS, "steps": steps, "repeats": repeats}
    for k, v in ts.items():
        out.update({k + "_step_us": float(np.median(v)), k + "_step_min_us": float(np.min(v)), k + "_step_max_us": float(np.max(v))})
    out["wolf_phc_over_qq"] = out["wolf_phc_step_us"] / out["qq_step_us"]
    b.close()
    return out


def trace_case(i, steps, repeats):
    from gym_soccer_littman94_amd import SoccerBatch
    w, h, slip, n = CASES[i]
    b = SoccerBatch(n, w, h, slip, seed=1994, autoreset=True)
    qs = learners(b)
    b.reset()
    for q in qs.values():
        q.run(200)
    for _ in range(repeats):
        for q in qs.values():
            q.run(steps)
    b.sync(); b.close()


def summarise(directory):
    """{trace file: {kernel: median / min / max device time in microseconds, dispatches}} of the learners' kernels"""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)):
        per = {}
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                short = next((k for k in ("phc_act_kernel", "phc_update_kernel", "q_act_kernel", "q_update_kernel") if k in name), None)
                if short is None:
                    continue
                mode = re.search(r"update_kernel(?:<|ILi)(\d)", name)
                if mode and mode.group(1) != "0":
                    continue                                    # MODE 1: creation, not a learner step
                per.setdefault(short, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        out[os.path.basename(path)] = {k: {"median_us": float(np.median(v)), "min_us": float(np.min(v)), "max_us": float(np.max(v)),
                                          "dispatches": len(v)} for k, v in per.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json"); ap.add_argument("--quick", action="store_true")
    ap.add_argument("--steps", type=int, default=1000); ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-case", type=int); ap.add_argument("--summarise")
    a = ap.parse_args()
    if a.trace_case is not None:
        trace_case(a.trace_case, min(a.steps, 200), a.repeats)
        return
    if a.summarise:
        out = {"kernels": summarise(a.summarise)}
        print(json.dumps(out, indent=1))
    else:
        rows = []
        for w, h, slip, n in (CASES[:1] if a.quick else CASES):
            rows.append(run(w, h, slip, n, a.steps, a.repeats))
            print(json.dumps(rows[-1]), flush=True)
        out = {"rows": rows}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
