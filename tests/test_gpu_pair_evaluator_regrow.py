"""The pair evaluators' one grow function (pair_buffers in csrc/soccer_pairs.hip) on every one of its triggers, for each of its
four buffer families.  Each evaluator's own regrow test starts with values=True, which leaves two triggers untried: a family that
grows by its policies alone, and values asked for of a family that was allocated without them.  On 5x4 at slip 0.2, a handle per
evaluator, four calls in order:

  1. 3 x 5 without values                        the first allocation: 15 pairs, less than a wave, no values buffer
  2. 9 x 8 without values, pairs_per_pass=64     more policies at the same stride: 72 pairs in two passes, the second ragged
  3. 9 x 8 with values, the library's passes     a larger stride (one pass of 128), and the values for the first time
  4. 3 x 5 with values                           nothing grows: a small matrix at the stride the large one left

Every result is held to the numpy restatement the evaluator's own module uses, to the bit, on sampled pairs (the first, 3 x 5's
last, and 63, 64 and 71 of 9 x 8: either side of the pass boundary, and the last of the ragged pass); calls 2 and 3, and 1 and 4,
are the same matrices and agree in every bit of what both return; the policy gradient's sums are the sequential sums of the pairs
that values=True returns (V, occupancy, q_a and q_b through the one transposed buffer).  The continuation probability is 0.5: no
solve takes more than 35 sweeps, three batches of the host's 16, and the restatements take a second or two."""
import os
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cross_play_np as cpn  # noqa: E402
import match_outcomes_np as mon  # noqa: E402
import policy_gradient_np as pgn  # noqa: E402
import test_gpu_occupancy as occ  # noqa: E402
import test_gpu_policy_gradient as grad  # noqa: E402
from test_gpu_best_response import oracle_lists, same_bits  # noqa: E402
from test_gpu_match_outcomes import KEYS as MATCH_KEYS, THETA, sets, starts_of  # noqa: E402

pytestmark = pytest.mark.gpu

PITCH = (5, 4, 0.2)
C = 0.5
SMALL, LARGE = (3, 5), (9, 8)
SAMPLE = [(0, 0), (1, 2), (2, 4), (7, 7), (8, 0), (8, 7)]
FLAT = [i * LARGE[1] + j for i, j in SAMPLE]
CROSS_KEYS = ("payoff", "iterations", "V")


def policies():
    return sets(*PITCH, *LARGE)


# ---- the four evaluators: the call as a dict, and the restatement of the sampled pairs as {key: [len(SAMPLE), ..]} -------------
def cross_call(b, A, B, values, ppp):
    return dict(zip(CROSS_KEYS, b.cross_play(A, B, THETA, C, pairs_per_pass=ppp, values=values)))


def cross_want(A, B):
    each = [cpn.cross_play(oracle_lists(*PITCH), starts_of(*PITCH), A[i], B[j], C, THETA) for i, j in SAMPLE]
    return {k: np.stack([r[n][0, 0] for r in each]) for n, k in enumerate(CROSS_KEYS)}


def match_call(b, A, B, values, ppp):
    return b.match_outcomes(A, B, THETA, C, pairs_per_pass=ppp, values=values)


def match_want(A, B):
    r = mon.match_outcomes(oracle_lists(*PITCH), starts_of(*PITCH), A, B, C, THETA, pairs=FLAT)
    return {k: r[k] for k in MATCH_KEYS}


def occupancy_call(b, A, B, values, ppp):
    return b.occupancy(A, B, THETA, C, features=occ.features_of(b.nS), values=values, pairs_per_pass=ppp)


def occupancy_want(A, B):
    r = occ.restate(*PITCH, A, B, C, pairs=FLAT)
    return {k: r[k] for k in occ.KEYS}


def gradient_call(b, A, B, values, ppp):
    return b.policy_gradient(A, B, THETA, C, values=values, pairs_per_pass=ppp)


def gradient_want(A, B):
    r = grad.restate_pairs(*PITCH, A, B, FLAT, C)
    return {k: r[k] for k in grad.PAIR_KEYS}


EVALUATORS = {"cross_play": (cross_call, cross_want), "match_outcomes": (match_call, match_want),
              "occupancy": (occupancy_call, occupancy_want), "policy_gradient": (gradient_call, gradient_want)}


@pytest.mark.parametrize("name", sorted(EVALUATORS))
def test_every_trigger_of_the_grow_function_leaves_the_restatement_s_bits(name):
    call, restate = EVALUATORS[name]
    A, B = policies()
    want = restate(A, B)
    b = SoccerBatch(1, *PITCH)
    calls = [("3 x 5 without values", SMALL, False, 0), ("9 x 8 without values in passes of 64", LARGE, False, 64),
             ("9 x 8 with values", LARGE, True, 0), ("3 x 5 with values", SMALL, True, 0)]
    got = [call(b, A[:n_a], B[:n_b], values, ppp) for _, (n_a, n_b), values, ppp in calls]
    b.close()
    for (what, (n_a, n_b), values, _), r in zip(calls, got):
        inside = [(n, i, j) for n, (i, j) in enumerate(SAMPLE) if i < n_a and j < n_b]
        assert len(inside) == (3 if (n_a, n_b) == SMALL else 6) and inside[-1][1:] == (n_a - 1, n_b - 1)
        keys = [k for k in want if k in r]
        assert len(keys) == len(want) if values else 2 <= len(keys) < len(want), (what, keys)
        for k in keys:
            for n, i, j in inside:
                same_bits(r[k][i, j], want[k][n], "%s of pair (%d, %d) of %s" % (k, i, j, what))
        if name == "policy_gradient" and values:
            for k, s in zip(grad.SUM_KEYS, pgn.reduce(r["occupancy"], r["q_a"], r["q_b"])):
                same_bits(r[k], s, "%s of %s from its pairs" % (k, what))
    # the same matrix whatever the buffers held and however it was split: every pair, and the policy gradient's sums
    for without, with_values in ((got[1], got[2]), (got[0], got[3])):
        assert set(without) < set(with_values)
        for k in without:
            same_bits(without[k], with_values[k], "%s without values against with values" % k)
    it = want["iterations"]
    print("%s at c = %.1f: the restated pairs take %d .. %d sweeps" % (name, C, it.min(), it.max()))
    assert 16 < it.max() <= 35                                          # more than one batch of sweeps; 0.5^34 < THETA
