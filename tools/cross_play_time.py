"""The cross-play matrix on the device (SoccerBatch.cross_play, values=False) against the same matrix through
SoccerBatch.evaluate_policies in chunks of 256 pairs, on one handle, gamma = 0.9, theta = 1e-10: 5x4 at slip 0 and 0.2 and
11x7 at slip 0.2, square matrices of 16, 64 and 256 policies a side.  Both are warmed up once, then timed alternately, repeat
by repeat; the median with minimum and maximum of the wall time is reported.  The policies are the uniform one, the two minimax
strategies and seeded Dirichlet rows in turn (tools/best_response_time.py).  The chunked side is skipped for a size once one of
its repeats takes more than --skip-after seconds, and the row says so.

    python tools/cross_play_time.py [--json OUT] [--repeats N] [--sizes 16,64,256] [--pitches 5x4:0,5x4:0.2,11x7:0.2]
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

GAMMA, THETA = 0.9, 1e-10


def chunked(b, A, B):
    """the matrix through evaluate_policies, 256 pairs a call: the kick-off values are left to the caller, as that call does"""
    na, nb = len(A), len(B)
    ii, jj = np.divmod(np.arange(na * nb), nb)
    its = np.zeros(na * nb, np.int64)
    for c in range(0, na * nb, 256):
        s = slice(c, c + 256)
        its[s] = b.evaluate_policies(A[ii[s]], B[jj[s]], THETA, GAMMA)[1]
    return its.reshape(na, nb)


def stats(x):
    return {"median_ms": float(np.median(x)) * 1e3, "min_ms": float(np.min(x)) * 1e3, "max_ms": float(np.max(x)) * 1e3}


def run(w, h, slip, sizes, repeats, skip_after):
    b = SoccerBatch(1, w, h, slip)
    pa, pb = b.minimax_value_iteration(THETA, GAMMA)[:2]
    rows = []
    for n in sizes:
        A, B = batch_of(pa, pb, n, seed=11), batch_of(pb, pa, n, seed=12)
        row = {"pitch": "%dx%d" % (w, h), "slip": slip, "nS": b.nS, "policies": n, "pairs": n * n,
               "uploaded_mb_cross": 2 * n * b.nS * 40 / 1e6, "uploaded_mb_chunked": 2 * n * n * b.nS * 40 / 1e6}
        its = b.cross_play(A, B, THETA, GAMMA)[1]                                   # warm-up
        skip = False
        t0 = time.perf_counter()
        ref = chunked(b, A, B)                                                      # warm-up
        first = time.perf_counter() - t0
        assert np.array_equal(its, ref)
        if first > skip_after:
            skip = True
            row["chunked_skipped"] = "one repeat took %.1f s" % first
            row["chunked"] = stats([first])
        new, old = [], []
        for _ in range(repeats):
            t0 = time.perf_counter(); b.cross_play(A, B, THETA, GAMMA); new.append(time.perf_counter() - t0)
            if not skip:
                t0 = time.perf_counter(); chunked(b, A, B); old.append(time.perf_counter() - t0)
        row.update(sweeps_min=int(its.min()), sweeps_max=int(its.max()), pair_sweeps=int(its.sum()), cross_play=stats(new))
        if not skip:
            row["chunked"] = stats(old)
        row["speedup_of_medians"] = row["chunked"]["median_ms"] / row["cross_play"]["median_ms"]
        row["us_per_sweep_cross"] = row["cross_play"]["median_ms"] * 1e3 / int(its.max())
        rows.append(row)
        print("%-5s slip %.1f %4d x %-4d  %3d..%3d sweeps  cross_play %9.2f ms (%.2f - %.2f)   chunked %10.2f ms (%.2f - %.2f)%s   x%.1f" % (
            row["pitch"], slip, n, n, row["sweeps_min"], row["sweeps_max"], row["cross_play"]["median_ms"], row["cross_play"]["min_ms"],
            row["cross_play"]["max_ms"], row["chunked"]["median_ms"], row["chunked"]["min_ms"], row["chunked"]["max_ms"],
            " [warm-up only]" if skip else "", row["speedup_of_medians"]), flush=True)
    b.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="16,64,256")
    ap.add_argument("--pitches", default="5x4:0,5x4:0.2,11x7:0.2")
    ap.add_argument("--skip-after", type=float, default=60.0)
    args = ap.parse_args()
    rows = []
    for spec in args.pitches.split(","):
        wh, slip = spec.split(":")
        w, h = (int(x) for x in wh.split("x"))
        rows += run(w, h, float(slip), [int(x) for x in args.sizes.split(",")], args.repeats, args.skip_after)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
