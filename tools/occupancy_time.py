"""SoccerBatch.occupancy beside SoccerBatch.match_outcomes and SoccerBatch.cross_play on one handle and the same policy sets
(tools/cross_play_time.py's), c = gamma = 0.9, theta = 1e-10, nothing but the [n, n] outputs asked for: 5x4 at slip 0 and 0.2,
16 and 64 policies a side, and 11x7 at slip 0.2, 16 a side.  All three are warmed up once, then timed alternately, repeat by
repeat (at least five); the median with minimum and maximum of the wall time is reported, and the time per sweep: the wall time
over the sweeps of the matrix's slowest pair, which is the number of sweep launches.  An occupancy sweep does three reads per
in-entry (two policy entries and D[s]) where a cross-play sweep does one gather per entry, and it walks only the entries that
do not end the game: ratio = (occupancy per sweep) / (cross_play per sweep).

    python tools/occupancy_time.py [--json OUT] [--repeats N] [--cases 5x4:0:16,5x4:0:64,5x4:0.2:16,5x4:0.2:64,11x7:0.2:16]
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
CALLS = ("cross_play", "match_outcomes", "occupancy")


def run(w, h, slip, sizes, repeats):
    b = SoccerBatch(1, w, h, slip)
    pa, pb = b.minimax_value_iteration(THETA, GAMMA)[:2]
    rows = []
    for n in sizes:
        A, B = batch_of(pa, pb, n, seed=11), batch_of(pb, pa, n, seed=12)
        call = {"cross_play": lambda: b.cross_play(A, B, THETA, GAMMA)[1], "match_outcomes": lambda: b.match_outcomes(A, B, THETA, GAMMA)["iterations"],
                "occupancy": lambda: b.occupancy(A, B, THETA, GAMMA)["iterations"]}
        sweeps = {k: int(call[k]().max()) for k in CALLS}                           # warm-up
        wall = {k: [] for k in CALLS}
        for _ in range(repeats):
            for k in CALLS:
                t0 = time.perf_counter(); call[k](); wall[k].append(time.perf_counter() - t0)
        row = {"pitch": "%dx%d" % (w, h), "slip": slip, "nS": b.nS, "policies": n, "pairs": n * n, "repeats": repeats}
        for k in CALLS:
            row["sweeps_" + k] = sweeps[k]
            row[k] = stats(wall[k])
            row[k + "_per_sweep"] = {key.replace("_ms", "_us_per_sweep"): v * 1e3 / sweeps[k] for key, v in stats(wall[k]).items()}
        for k in ("cross_play", "match_outcomes"):
            row["ratio_to_" + k] = row["occupancy_per_sweep"]["median_us_per_sweep"] / row[k + "_per_sweep"]["median_us_per_sweep"]
        rows.append(row)
        print("%-5s slip %.1f %4d x %-4d  " % (row["pitch"], slip, n, n) + "   ".join(
            "%s %3d sweeps %9.2f us/sweep (%.2f - %.2f)" % (k, sweeps[k], row[k + "_per_sweep"]["median_us_per_sweep"],
                                                            row[k + "_per_sweep"]["min_us_per_sweep"], row[k + "_per_sweep"]["max_us_per_sweep"])
            for k in CALLS) + "   x%.2f of cross_play, x%.2f of match_outcomes" % (row["ratio_to_cross_play"], row["ratio_to_match_outcomes"]),
            flush=True)
    b.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", default="5x4:0:16,5x4:0:64,5x4:0.2:16,5x4:0.2:64,11x7:0.2:16")
    args = ap.parse_args()
    assert args.repeats >= 5, "at least five repeats"
    rows = []
    for spec in args.cases.split(","):
        wh, slip, n = spec.split(":")
        w, h = (int(x) for x in wh.split("x"))
        rows += run(w, h, float(slip), [int(n)], args.repeats)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
