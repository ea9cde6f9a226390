"""Minimax value iteration on the device (SoccerBatch.minimax_value_iteration), gamma = 0.9, theta = 1e-10:
sweep count, device time per sweep, wall time to convergence on a fresh handle (list construction included) and on a warm
one, bytes of list data one sweep reads, the fraction of stage games the saddle-point path solves — on 5x4 at slip 0 and
0.2 and on the largest reference pitch, 11x7 at slip 0.2 — and, where scipy can be imported, what solving the same
per-state games with scipy.optimize.linprog (HiGHS) on the host costs.

    python tools/minimax_time.py [--json OUT]
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


def list_bytes(b):
    """bytes of the (state, joint action) lists one sweep reads: 16-byte entries padded to four per list, plus offsets"""
    count = b.transitions()[0]
    lut, goal_value, _ = b.tables()
    obs_of = np.where(goal_value != 0, 0, lut.astype(np.int64))
    tuple_of = np.full(b.nS, -1, np.int64)
    for f in np.flatnonzero(lut != 0xFFFF):
        tuple_of[obs_of[f]] = f                                         # the last goal tuple owns index 0
    c = count[tuple_of]
    return int(((c + 3) // 4 * 4).sum() * 16 + (b.nS * 25 + 1) * 4)


def saddle_mask(Q):
    return Q.min(2).max(1) == Q.max(1).min(1)


def linprog_cost(Q, limit):
    try:
        from scipy.optimize import linprog
    except ImportError:
        return None
    idx = np.flatnonzero(~saddle_mask(Q))[:limit]
    t0 = time.perf_counter()
    for s in idx:
        A = Q[s]
        c = np.zeros(6); c[5] = -1.0
        r = linprog(c, A_ub=np.hstack([-A.T, np.ones((5, 1))]), b_ub=np.zeros(5), A_eq=np.array([[1.0] * 5 + [0.0]]),
                    b_eq=np.array([1.0]), bounds=[(0, None)] * 5 + [(None, None)], method="highs")
        assert r.status == 0
    return (time.perf_counter() - t0) / max(len(idx), 1), len(idx)


def run(w, h, slip, lp_limit):
    t0 = time.perf_counter()
    b = SoccerBatch(1, w, h, slip)
    t_create = time.perf_counter() - t0
    t0 = time.perf_counter()
    pa, pb, V, Q, k = b.minimax_value_iteration(THETA, GAMMA)
    fresh = time.perf_counter() - t0                                    # includes enumerating and uploading the lists
    warm, ev = [], []
    for _ in range(3):
        b.timer_start()
        t0 = time.perf_counter()
        again = b.minimax_value_iteration(THETA, GAMMA)
        warm.append(time.perf_counter() - t0)
        ev.append(b.timer_stop())
        assert again[4] == k and np.array_equal(again[2], V)
    nonsad = int((~saddle_mask(Q)).sum())
    row = {"pitch": "%dx%d" % (w, h), "slip": slip, "nS": b.nS, "sweeps": k,
           "create_ms": t_create * 1e3, "fresh_solve_ms": fresh * 1e3, "warm_solve_ms": min(warm) * 1e3,
           "list_build_ms": (fresh - min(warm)) * 1e3,
           "stream_ms_per_sweep": min(ev) / k, "wall_ms_per_sweep": min(warm) * 1e3 / k,
           "list_bytes_per_sweep": list_bytes(b), "saddle_fraction": 1.0 - nonsad / b.nS, "nonsaddle_states": nonsad}
    lp = linprog_cost(Q, lp_limit)
    if lp is None:
        row["linprog"] = "scipy cannot be imported here: not timed"
    else:
        row["linprog_ms_per_game"] = lp[0] * 1e3
        row["linprog_games_timed"] = lp[1]
        row["linprog_ms_per_sweep_est"] = lp[0] * 1e3 * nonsad
    b.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--lp-limit", type=int, default=400, help="non-saddle games timed with linprog per pitch")
    args = ap.parse_args()
    rows = [run(5, 4, 0.0, args.lp_limit), run(5, 4, 0.2, args.lp_limit), run(11, 7, 0.2, args.lp_limit)]
    for r in rows:
        print("%-5s slip %.1f nS %5d: %3d sweeps, fresh %.1f ms (lists %.1f ms), warm %.2f ms, %.1f us/sweep on the stream "
              "(%.1f us wall), %.2f MB lists/sweep, saddle %.1f %%" % (
                  r["pitch"], r["slip"], r["nS"], r["sweeps"], r["fresh_solve_ms"], r["list_build_ms"], r["warm_solve_ms"],
                  r["stream_ms_per_sweep"] * 1e3, r["wall_ms_per_sweep"] * 1e3, r["list_bytes_per_sweep"] / 1e6,
                  100 * r["saddle_fraction"]))
        if "linprog_ms_per_game" in r:
            print("      linprog (HiGHS, host): %.2f ms per non-saddle game (%d timed) -> ~%.0f ms per sweep over %d such states" % (
                r["linprog_ms_per_game"], r["linprog_games_timed"], r["linprog_ms_per_sweep_est"], r["nonsaddle_states"]))
        else:
            print("      " + r["linprog"])
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
