"""The meta-game solve on the device (SoccerBatch.solve_meta_game, the matrix already on the host) against
scipy.optimize.linprog(method="highs") on the same matrices on the host, which is what a user has without it:
  * 256 games of 64 x 64 in one call (the LDS kernel, a workgroup per game);
  * 256 x 256 and 1024 x 1024 (the global kernels), uniform(-1, 1) entries and a rank-3 product, each at pivots_per_sync of
    16, 64, 256 and the library's choice;
  * single uniform games of 4 .. 256 a side, to find the size below which the host solver wins.
Each is warmed up once, then timed --repeats times; the median with minimum and maximum of the wall time is reported, with the
pivot counts, the statuses and the widest bracket.  A host solve that takes more than --skip-after seconds is timed once.
With --trace the tool runs itself under rocprofv3 --kernel-trace --stats on the 256 x 256 uniform game alone and reports the
time per meta_select_kernel and meta_update_kernel launch.

    python tools/meta_game_time.py [--json OUT] [--repeats N] [--no-large] [--trace]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gym_soccer_littman94_amd import SoccerBatch  # noqa: E402


def matrix(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.uniform(-1.0, 1.0, (n, n))
    return rng.standard_normal((n, 3)) @ rng.standard_normal((3, n))               # "rank3"


def highs(A):
    from scipy.optimize import linprog
    n_a, n_b = A.shape
    c = np.zeros(n_a + 1); c[-1] = -1.0
    A_eq = np.ones((1, n_a + 1)); A_eq[0, -1] = 0.0
    res = linprog(c, A_ub=np.hstack([-A.T, np.ones((n_b, 1))]), b_ub=np.zeros(n_b), A_eq=A_eq, b_eq=[1.0],
                  bounds=[(0, None)] * n_a + [(None, None)], method="highs")
    return float(res.x[-1])


def stats(x):
    return {"median_ms": float(np.median(x)) * 1e3, "min_ms": float(np.min(x)) * 1e3, "max_ms": float(np.max(x)) * 1e3}


def fmt(s):
    return "%10.2f ms (%.2f - %.2f)" % (s["median_ms"], s["min_ms"], s["max_ms"])


def timed(fn, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter(); fn(); out.append(time.perf_counter() - t0)
    return out


def solve(b, A, **kw):
    """status 3 raises; the timing tool wants the dict either way"""
    try:
        return b.solve_meta_game(A, **kw)
    except RuntimeError as e:
        return e.results


def case(b, name, A, repeats, skip_after, sweep):
    games = A.reshape((-1,) + A.shape[-2:])
    r = solve(b, A)                                                                 # warm-up
    row = {"case": name, "games": len(games), "n_a": A.shape[-2], "n_b": A.shape[-1],
           "pivots_min": int(np.min(r["pivots"])), "pivots_max": int(np.max(r["pivots"])),
           "status": sorted(set(np.atleast_1d(r["status"]).tolist())), "gap_max": float(np.max(r["gap"])),
           "device": stats(timed(lambda: solve(b, A), repeats))}
    if sweep:
        row["pivots_per_sync"] = {str(p): stats(timed(lambda: solve(b, A, path=2, pivots_per_sync=p), repeats)) for p in (16, 64, 256)}
    t0 = time.perf_counter()
    ref = [highs(g) for g in games]
    first = time.perf_counter() - t0
    row["host_highs"] = stats([first] if first > skip_after else timed(lambda: [highs(g) for g in games], repeats))
    row["host_repeats"] = 1 if first > skip_after else repeats
    lo, hi = np.atleast_1d(r["lo"]), np.atleast_1d(r["hi"])
    row["highs_inside_bracket"] = bool(all(lo[g] - 1e-7 * max(1, np.abs(games[g]).max()) <= ref[g] <= hi[g] + 1e-7 * max(1, np.abs(games[g]).max())
                                           for g in range(len(games))))
    row["host_over_device"] = row["host_highs"]["median_ms"] / row["device"]["median_ms"]
    print("%-22s pivots %5d..%-5d status %s gap %.1e  device %s   HiGHS %s   x%.2f" % (
        name, row["pivots_min"], row["pivots_max"], row["status"], row["gap_max"], fmt(row["device"]), fmt(row["host_highs"]),
        row["host_over_device"]), flush=True)
    if sweep:
        print("    pivots_per_sync: " + "   ".join("%s %s" % (p, fmt(s)) for p, s in row["pivots_per_sync"].items()), flush=True)
    return row


def trace():
    """this tool under rocprofv3 on one 256 x 256 solve: mean time per select and per update launch"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--only-solve"]
        try:
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        except (OSError, subprocess.SubprocessError) as e:
            return {"not_measured": "rocprofv3 failed: %s" % type(e).__name__}
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                name = r.get("Name", "")
                for k in ("meta_select_kernel", "meta_update_kernel", "meta_setup_kernel", "meta_finish_kernel", "meta_count_kernel"):
                    if k in name:
                        out[k] = {"calls": int(r["Calls"]), "mean_us": float(r["AverageNs"]) / 1e3, "total_ms": float(r["TotalDurationNs"]) / 1e6}
        return out or {"not_measured": "no kernel statistics were written"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-after", type=float, default=5.0)
    ap.add_argument("--no-large", action="store_true", help="leave the 1024 x 1024 games out")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--only-solve", action="store_true", help="one warmed-up 256 x 256 solve and nothing else (what --trace profiles)")
    args = ap.parse_args()
    b = SoccerBatch(1, 5, 4, 0.0)
    if args.only_solve:
        A = matrix("uniform", 256, 1)
        solve(b, A, path=2); solve(b, A, path=2)
        b.close()
        return
    rows = [case(b, "64x64 x 256 games", np.stack([matrix("uniform", 64, 100 + g) for g in range(256)]), args.repeats, args.skip_after, False)]
    for n in (256,) if args.no_large else (256, 1024):
        for kind in ("uniform", "rank3"):
            rows.append(case(b, "%dx%d %s" % (n, n, kind), matrix(kind, n, 1), args.repeats, args.skip_after, True))
    single = [case(b, "single %dx%d" % (n, n), matrix("uniform", n, 2), args.repeats, args.skip_after, False) for n in (4, 8, 16, 32, 64, 128, 256)]
    wins = [r["n_a"] for r in single if r["host_over_device"] < 1.0]
    out = {"cases": rows, "single_games": single, "host_solver_wins_up_to": max(wins) if wins else 0,
           "kernel_trace_256x256_uniform": trace() if args.trace else {"not_measured": "run with --trace"}}
    print("the host solver wins up to %d a side; kernel trace: %s" % (out["host_solver_wins_up_to"], out["kernel_trace_256x256_uniform"]))
    b.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
