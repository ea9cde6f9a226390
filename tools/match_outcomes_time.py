"""SoccerBatch.match_outcomes against SoccerBatch.cross_play on one handle and the same policy sets (tools/cross_play_time.py's),
c = gamma = 0.9, theta = 1e-10, values=False: 5x4 at slip 0 and 0.2 and 11x7 at slip 0.2, square matrices of 16, 64 and 256
policies a side.  Both are warmed up once, then timed alternately, repeat by repeat (at least five); the median with minimum and
maximum of the wall time is reported, and the time per sweep: the wall time over the sweeps of the matrix's slowest pair, which
is the number of sweep launches.  A three-channel sweep reads every list entry once for its three sums, so the question is how
far below three cross-play sweeps it stays: ratio = (match_outcomes per sweep) / (cross_play per sweep).

    python tools/match_outcomes_time.py [--json OUT] [--repeats N] [--sizes 16,64,256] [--pitches 5x4:0,5x4:0.2,11x7:0.2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gym_soccer_littman94_amd import SoccerBatch  # noqa: E402
from best_response_time import batch_of  # noqa: E402
from cross_play_time import stats  # noqa: E402

GAMMA, THETA = 0.9, 1e-10


def run(w, h, slip, sizes, repeats):
    b = SoccerBatch(1, w, h, slip)
    pa, pb = b.minimax_value_iteration(THETA, GAMMA)[:2]
    rows = []
    for n in sizes:
        A, B = batch_of(pa, pb, n, seed=11), batch_of(pb, pa, n, seed=12)
        k_cross = int(b.cross_play(A, B, THETA, GAMMA)[1].max())                    # warm-up
        r = b.match_outcomes(A, B, THETA, GAMMA)                                    # warm-up
        k_match = int(r["iterations"].max())
        cross, match = [], []
        for _ in range(repeats):
            t0 = time.perf_counter(); b.cross_play(A, B, THETA, GAMMA); cross.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); b.match_outcomes(A, B, THETA, GAMMA); match.append(time.perf_counter() - t0)
        per = lambda x, k: {key.replace("_ms", "_us_per_sweep"): v * 1e3 / k for key, v in stats(x).items()}   # noqa: E731
        row = {"pitch": "%dx%d" % (w, h), "slip": slip, "nS": b.nS, "policies": n, "pairs": n * n, "repeats": repeats,
               "sweeps_cross": k_cross, "sweeps_match": k_match, "cross_play": stats(cross), "match_outcomes": stats(match),
               "cross_play_per_sweep": per(cross, k_cross), "match_outcomes_per_sweep": per(match, k_match)}
        row["ratio_per_sweep"] = row["match_outcomes_per_sweep"]["median_us_per_sweep"] / row["cross_play_per_sweep"]["median_us_per_sweep"]
        rows.append(row)
        c, m = row["cross_play_per_sweep"], row["match_outcomes_per_sweep"]
        print("%-5s slip %.1f %4d x %-4d  cross_play %3d sweeps %9.2f us/sweep (%.2f - %.2f)   match_outcomes %3d sweeps %9.2f us/sweep "
              "(%.2f - %.2f)   x%.2f" % (row["pitch"], slip, n, n, k_cross, c["median_us_per_sweep"], c["min_us_per_sweep"],
                                         c["max_us_per_sweep"], k_match, m["median_us_per_sweep"], m["min_us_per_sweep"],
                                         m["max_us_per_sweep"], row["ratio_per_sweep"]), flush=True)
    b.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="16,64,256")
    ap.add_argument("--pitches", default="5x4:0,5x4:0.2,11x7:0.2")
    args = ap.parse_args()
    assert args.repeats >= 5, "at least five repeats"
    rows = []
    for spec in args.pitches.split(","):
        wh, slip = spec.split(":")
        w, h = (int(x) for x in wh.split("x"))
        rows += run(w, h, float(slip), [int(x) for x in args.sizes.split(",")], args.repeats)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
