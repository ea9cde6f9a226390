"""SoccerBatch.policy_gradient beside SoccerBatch.cross_play followed by SoccerBatch.occupancy on one handle and the same policy
sets (tools/cross_play_time.py's), gamma = 0.9, theta = 1e-10: 5x4 at slip 0 and 0.2, 16 and 64 policies a side, and 11x7 at slip
0.2, 16 a side.  The call asks for payoff, both gradients, both reaches and the sweep counts; the two calls of the baseline for
their [n, n] outputs alone (payoff, length, sweep counts): they do strictly less.  One warm-up of
each, then at least five repeats alternating between the two; the median with minimum and maximum of the wall time is reported.
The call adds one launch of action_values_kernel, about one sweep's work, and two launches of gradient_reduce_kernel to the
k_V + k_D sweeps of the baseline and saves one upload of the policies: `allowed` is the baseline's own min-max spread plus
2 / (k_V + k_D) of its median, and `over` says whether the call's median exceeds the baseline's by more than that.
Then GradientPlay.run(20) beside twenty rounds of the public call plus the numpy update (tests/policy_gradient_np.step), 16 x 16
on 5x4 at slip 0.2: steps per second of run have no earlier figure to compare with.

    python tools/policy_gradient_time.py [--json OUT] [--repeats N] [--cases 5x4:0:16,5x4:0:64,5x4:0.2:16,5x4:0.2:64,11x7:0.2:16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gym_soccer_littman94_amd import SoccerBatch  # noqa: E402
from best_response_time import batch_of  # noqa: E402
from cross_play_time import stats  # noqa: E402
import policy_gradient_np as pgn  # noqa: E402

GAMMA, THETA = 0.9, 1e-10
CALLS = ("policy_gradient", "cross_play_then_occupancy")


def run(w, h, slip, n, repeats):
    b = SoccerBatch(1, w, h, slip)
    pa, pb = b.minimax_value_iteration(THETA, GAMMA)[:2]
    A, B = batch_of(pa, pb, n, seed=11), batch_of(pb, pa, n, seed=12)

    def two_calls():
        it = b.cross_play(A, B, THETA, GAMMA)[1]
        return np.stack([it, b.occupancy(A, B, THETA, GAMMA)["iterations"]], -1)

    call = {"policy_gradient": lambda: b.policy_gradient(A, B, THETA, GAMMA)["iterations"], "cross_play_then_occupancy": two_calls}
    its = {k: call[k]() for k in CALLS}                                 # warm-up
    assert (its["policy_gradient"] == its["cross_play_then_occupancy"]).all()
    sweeps = int(its["policy_gradient"][..., 0].max() + its["policy_gradient"][..., 1].max())     # the sweep launches of either
    wall = {k: [] for k in CALLS}
    for _ in range(repeats):
        for k in CALLS:
            t0 = time.perf_counter(); call[k](); wall[k].append(time.perf_counter() - t0)
    b.close()
    row = {"pitch": "%dx%d" % (w, h), "slip": slip, "nS": b.nS, "policies": n, "pairs": n * n, "repeats": repeats, "sweeps": sweeps}
    for k in CALLS:
        row[k] = stats(wall[k])
    base = row["cross_play_then_occupancy"]
    row["allowed_ms"] = (base["max_ms"] - base["min_ms"]) + 2.0 / sweeps * base["median_ms"]
    row["excess_ms"] = row["policy_gradient"]["median_ms"] - base["median_ms"]
    row["over"] = bool(row["excess_ms"] > row["allowed_ms"])
    print("%-5s slip %.1f %4d x %-4d %4d sweeps   " % (row["pitch"], slip, n, n, sweeps) + "   ".join(
        "%s %9.2f ms (%.2f - %.2f)" % (k, row[k]["median_ms"], row[k]["min_ms"], row[k]["max_ms"]) for k in CALLS)
        + "   excess %.2f ms, allowed %.2f ms%s" % (row["excess_ms"], row["allowed_ms"], "  OVER" if row["over"] else ""), flush=True)
    return row


def run_learner(repeats, n=16, steps=20, gamma=GAMMA, theta=THETA):
    w, h, slip = 5, 4, 0.2
    b = SoccerBatch(1, w, h, slip)
    pa, pb = b.minimax_value_iteration(THETA, GAMMA)[:2]
    A, B = batch_of(pa, pb, n, seed=11), batch_of(pb, pa, n, seed=12)
    kw = dict(n_a=n, n_b=n, discount_factor=gamma, eta_a=1.0, eta_b=1.0, optimism=1.0, normalize=True, theta=theta)

    def resident():
        g = b.gradient_play(pi_a=A, pi_b=B, **kw)
        g.run(steps)
        r = g.read()
        g.close()
        return r["pi_a"], r["pi_b"]

    def rounds():
        x, y, prev_a, prev_b = A, B, np.zeros(A.shape), np.zeros(B.shape)
        for t in range(steps):
            r = b.policy_gradient(x, y, theta, gamma, normalize=True)
            x, y, prev_a, prev_b = pgn.step(x, y, r["grad_a"], r["grad_b"], prev_a, prev_b, t == 0, 1.0, 1.0, 1.0)
        return x, y

    call = {"run": resident, "rounds_of_the_public_call": rounds}
    first = {k: call[k]() for k in call}                                # warm-up
    assert all((np.ascontiguousarray(p).view(np.int64) == np.ascontiguousarray(q).view(np.int64)).all()
               for p, q in zip(first["run"], first["rounds_of_the_public_call"]))
    wall = {k: [] for k in call}
    for _ in range(repeats):
        for k in call:
            t0 = time.perf_counter(); call[k](); wall[k].append(time.perf_counter() - t0)
    b.close()
    row = {"pitch": "5x4", "slip": slip, "policies": n, "steps": steps, "repeats": repeats,
           "note": "steps per second of run have no earlier figure to compare with"}
    for k in call:
        row[k] = stats(wall[k])
        row[k + "_steps_per_s"] = steps / (row[k]["median_ms"] * 1e-3)
    print("gradient play, %d x %d on 5x4 slip %.1f, %d steps:   " % (n, n, slip, steps) + "   ".join(
        "%s %9.2f ms (%.2f - %.2f), %.1f steps/s" % (k, row[k]["median_ms"], row[k]["min_ms"], row[k]["max_ms"], row[k + "_steps_per_s"])
        for k in call), flush=True)
    return row


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
        rows.append(run(w, h, float(slip), int(n), args.repeats))
    out = {"gamma": GAMMA, "theta": THETA, "calls": rows, "gradient_play": run_learner(args.repeats)}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
