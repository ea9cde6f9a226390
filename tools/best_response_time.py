"""Best responses to mixed policies on the device (SoccerBatch.best_response), gamma = 0.9, theta = 1e-10: per pitch, slip
and batch size (1, 16, 256 policies) the sweep count of the slowest policy, device and wall time per sweep on a warm handle,
and the solve time on a fresh handle (list construction and buffer allocation included) — on 5x4 at slip 0 and 0.2 and on
the largest reference pitch, 11x7 at slip 0.2.  A batch holds the uniform policy, the two minimax strategies and seeded
Dirichlet rows in turn, so it mixes policies that need about 50 sweeps with policies that need about 180.  The Shapley sweep
of the same handle (SoccerBatch.minimax_value_iteration, tools/minimax_time.py) is timed next to it as the yardstick.

    python tools/best_response_time.py [--json OUT] [--repeats N] [--batches 1,16,256]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_soccer_littman94_amd import SoccerBatch  # noqa: E402

GAMMA, THETA = 0.9, 1e-10


def batch_of(pa, pb, n, seed=11):
    rng = np.random.default_rng(seed)
    nS = pa.shape[0]
    kinds = [lambda: np.full((nS, 5), 0.2), lambda: pa, lambda: pb, lambda: rng.dirichlet(np.ones(5), nS)]
    return np.stack([kinds[i % 4]() for i in range(n)]) if n > 1 else pa[None]


def timed(b, call, repeats):
    wall, ev, out = [], [], None
    for _ in range(repeats):
        b.timer_start()
        t0 = time.perf_counter()
        out = call()
        wall.append(time.perf_counter() - t0)
        ev.append(b.timer_stop())
    return out, float(np.median(wall)), float(np.median(ev)) * 1e-3, [w * 1e3 for w in wall]


def run(w, h, slip, sizes, repeats):
    b = SoccerBatch(1, w, h, slip)
    pa, pb, V, _, k = b.minimax_value_iteration(THETA, GAMMA)
    _, wall, ev, _ = timed(b, lambda: b.minimax_value_iteration(THETA, GAMMA), repeats)
    rows = [{"pitch": "%dx%d" % (w, h), "slip": slip, "nS": b.nS, "what": "minimax_value_iteration", "policies": 1, "sweeps": k,
             "warm_solve_ms": wall * 1e3, "wall_us_per_sweep": wall * 1e6 / k, "stream_us_per_sweep": ev * 1e6 / k}]
    b.close()
    for n in sizes:
        pol = batch_of(pa, pb, n)
        for player in (0, 1):
            t0 = time.perf_counter()
            f = SoccerBatch(1, w, h, slip)
            t_create = time.perf_counter() - t0
            t0 = time.perf_counter()
            first = f.best_response(pol, player, THETA, GAMMA)
            fresh = time.perf_counter() - t0
            out, wall, ev, walls = timed(f, lambda: f.best_response(pol, player, THETA, GAMMA), repeats)
            assert all(np.array_equal(x, y) for x, y in zip(out, first))
            its = out[3]
            k = int(its.max())
            launches = -(-k // 16) * 16                                  # sweeps are enqueued sixteen at a time
            rows.append({"pitch": "%dx%d" % (w, h), "slip": slip, "nS": f.nS, "what": "best_response", "fixed_player": "AB"[player],
                         "policies": n, "sweeps": k, "sweeps_min": int(its.min()), "policy_sweeps": int(its.sum()), "launches": launches,
                         "create_ms": t_create * 1e3, "fresh_solve_ms": fresh * 1e3, "warm_solve_ms": wall * 1e3,
                         "warm_solve_ms_all": walls, "wall_us_per_sweep": wall * 1e6 / k, "stream_us_per_sweep": ev * 1e6 / k,
                         "wall_us_per_policy_sweep": wall * 1e6 / int(its.sum())})
            f.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", default="1,16,256")
    args = ap.parse_args()
    sizes = [int(x) for x in args.batches.split(",")]
    rows = []
    for w, h, slip in ((5, 4, 0.0), (5, 4, 0.2), (11, 7, 0.2)):
        rows += run(w, h, slip, sizes, args.repeats)
    for r in rows:
        head = "%-5s slip %.1f nS %5d  %-24s" % (r["pitch"], r["slip"], r["nS"], r["what"] + (" vs " + r["fixed_player"] if "fixed_player" in r else ""))
        if r["what"] == "best_response":
            print("%s %3d policies: %3d sweeps (min %3d), fresh %.1f ms, warm %.2f ms, %.1f us/sweep wall (%.1f on the stream), "
                  "%.2f us per policy and sweep" % (head, r["policies"], r["sweeps"], r["sweeps_min"], r["fresh_solve_ms"], r["warm_solve_ms"],
                                                    r["wall_us_per_sweep"], r["stream_us_per_sweep"], r["wall_us_per_policy_sweep"]))
        else:
            print("%s                %3d sweeps, warm %.2f ms, %.1f us/sweep wall (%.1f on the stream)" % (
                head, r["sweeps"], r["warm_solve_ms"], r["wall_us_per_sweep"], r["stream_us_per_sweep"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
