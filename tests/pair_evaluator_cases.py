"""The cases of the pair evaluators' shape and edge tests (soccer_match_outcomes, soccer_occupancy, soccer_policy_gradient and
soccer_gradient_play_*): the eight pitches with their continuation probability, 2 x 3 matrix, features and weights; and on 5x4 at
slips 0.0 and 0.2 the parameter ends, the unusual rows, the matrices at the limit of 1024 policies a side and the three matrices
that each call's own pairs_per_pass has to split — with the restatements' lists, kick-off states and in-lists they are solved over,
and the three restatements run on one input (three_calls).  tests/two_player_cases.py supplies what the two-player edge tests
already define.  No GPU is needed here: tests/test_pair_evaluator_cases_np.py shows on the restatements alone that each case
reaches its path, tests/test_gpu_pair_evaluator_shapes.py and tests/test_gpu_pair_evaluator_edges.py hold the device to the
restatements on the same inputs."""
import functools

import numpy as np

from oracle.oracle import Oracle

import best_response_np as brn
import cross_play_np as cpn
import match_outcomes_np as mon
import occupancy_np as ocn
import policy_gradient_np as pgn
from minimax_q_np import shapley_lists
from two_player_cases import NS, pass_policies, pitch

THETA = 1e-10
# ---- the pitches: width, height, slip (test_gpu_two_player_shapes.PITCHES) ------------------------------------------------
PITCHES = [(5, 4, 0.0), (6, 4, 0.2), (6, 5, 0.2), (7, 5, 1.0), (5, 9, 0.3), (8, 7, 0.0), (11, 7, 0.2), (13, 8, 0.1)]
IDS = ["%dx%d" % p[:2] for p in PITCHES]
# per pitch (the longest in-list with its padding, the out-lists' width K), as the restatement builds them: the three regimes of
# slip 0, an ordinary slip and slip 1
IN_LISTS = {(5, 4, 0.0): (40, 4), (6, 4, 0.2): (344, 15), (6, 5, 0.2): (344, 15), (7, 5, 1.0): (152, 7), (5, 9, 0.3): (344, 15),
            (8, 7, 0.0): (40, 4), (11, 7, 0.2): (344, 15), (13, 8, 0.1): (344, 15)}
LARGEST = (13, 8, 0.1)                  # 21 425 states: its lists alone take a CPU some 20 s, so the CPU module leaves it out
W_A, W_B = np.array([0.25, 1.0 / 3.0]), np.array([0.1, 7.0, 1.0 / 3.0])        # non-dyadic, no unit sum
N_F = 3


def n_states(w, h):
    return 2 * w * h * (w * h - 1) + 1


def kickoffs(h):
    """Rules::build: the carrier starts on either middle row of an even height"""
    return 4 if h % 2 == 0 else 2


def discount(w, h):
    """test_gpu_two_player_shapes.discount: 0.9 up to 7x5, 0.5 on the larger pitches.  At 0.5 no channel of any of the three
    solves moves by more than 0.5^(k-1) in sweep k (|V_1|, |W_1| <= 1, L_1 = 1, sum D_1 = 1), below 1e-10 from k = 35 on"""
    return 0.9 if n_states(w, h) <= n_states(7, 5) else 0.5


def features_of(nS, n_f=N_F):
    """test_gpu_occupancy.features_of: an indicator of every third state, then random weights in [-1, 1)"""
    rng = np.random.default_rng(9)
    return np.concatenate([(np.arange(nS) % 3 == 1).astype(np.float64)[None], rng.random((n_f - 1, nS)) * 2 - 1])


class Shape:
    """one pitch: the oracle's two-player lists, kick-off states and in-lists, and the 2 x 3 matrix of
    test_gpu_two_player_shapes.Game (the same draws in the same order, so the pair (1, 1) is one-hot against itself)"""

    def __init__(self, w, h, slip):
        self.w, self.h, self.slip, self.c = w, h, slip, discount(w, h)
        orc = Oracle(w, h, slip, n=1, seed=0)
        self.nS = nS = orc.nS
        self.lists = shapley_lists(orc)
        self.starts = cpn.isd_obs(orc)
        self.inl = ocn.in_lists_of(self.lists)
        rng = np.random.default_rng(w * 100 + h)
        rng.uniform(-1, 1, nS)                                  # (that module's input of a backup, drawn first)
        self.A = np.stack([rng.dirichlet(np.full(5, 0.2), nS), brn.onehot(rng.integers(0, 5, nS))])
        self.B = np.stack([np.full((nS, 5), 0.2), self.A[1], rng.dirichlet(np.ones(5), nS)])
        self.F = features_of(nS)
        self.ref = {}

    def longest_in_list(self):
        return int(np.diff(self.inl[0]).max())

    def restated(self):
        """{"match", "occupancy", "gradient"}: the three restatements of the 2 x 3 matrix, computed once"""
        if not self.ref:
            lists, starts, A, B, c = self.lists, self.starts, self.A, self.B, self.c
            self.ref["match"] = mon.match_outcomes(lists, starts, A, B, c, THETA)
            self.ref["occupancy"] = ocn.occupancy(lists, starts, A, B, c, THETA, features=self.F, inl=self.inl)
            self.ref["gradient"] = pgn.policy_gradient(lists, starts, A, B, c, THETA, W_A, W_B, True, inl=self.inl)
        return self.ref


_shapes = {}


def shape(w, h, slip):
    if (w, h, slip) not in _shapes:
        _shapes[(w, h, slip)] = Shape(w, h, slip)
    return _shapes[(w, h, slip)]


def forget_shapes():
    """drops the pitches' lists and references (13x8's lists alone are a quarter of a GB)"""
    _shapes.clear()


# ---- the edges, on 5x4 at two_player_cases.SLIPS ------------------------------------------------------------------------------
UNUSUAL_SWEEPS = 230                    # what the unusual rows stop under at 0.9 in every call (0.9^219 < 1e-10 <= 0.9^218, and a margin)
PLAY = dict(eta_a=1.0, eta_b=1.0, optimism=0.5, normalize=True)         # gradient play from the unusual rows, two steps
LIMIT_SHAPES = [(1024, 1), (1, 1024), (1024, 2)]
LIMIT_C = 0.5
SPAN_SHAPE, SPAN_PASSES = (67, 7), (64, 128)                            # the policy gradient's columns spanning passes
# the library's own pass split (soccer_pairs.hip: what soccer_occupancy, soccer_match_outcomes and gradient_solve hand to pass_pairs)
PASS_BYTES = {"occupancy": 16, "match": 48, "gradient": 112}            # bytes a pair and state of one pass: 2 D; 2 x 3 F; 2 V, 2 D, 10 Q
PASS_PAIRS = {k: 2 ** 30 // (v * NS) // 64 * 64 for k, v in PASS_BYTES.items()}
PASS_NB = {"occupancy": 87, "match": 29, "gradient": 13}                # x 1024 of pass_policies(): just above one pass
# 0.05: no channel moves by more than 0.05^(k-1) in sweep k, below 1e-10 from k = 9 on, for every pair of policies
PASS_C, PASS_SWEEPS = 0.05, 9


@functools.lru_cache(maxsize=None)
def in_lists(slip):
    return ocn.in_lists_of(pitch(slip)[0])


@functools.lru_cache(maxsize=None)
def pool():
    """two_player_cases.pass_policies(): (1024, 87) policies of uniform, Dirichlet(1), Dirichlet(0.2) and one-hot rows in turn"""
    return pass_policies()


def weights(n):
    """non-uniform, non-dyadic, no unit sum"""
    return (1.0 + np.arange(n) % 7) / 3.0


def limit_policies(n_a, n_b):
    A, B = pool()
    return (A[:n_a], B[:n_b]) if n_a > 1 else (B[3:4], A[:n_b])


def pass_matrix(call):
    A, B = pool()
    return A, B[:PASS_NB[call]]


def pass_sample(call):
    """flat pairs of the call's pass-split matrix: the first, the pairs either side of the pass boundary, the ends of the second
    pass's first wave, the last, and a dozen more at an odd stride"""
    per, total = PASS_PAIRS[call], 1024 * PASS_NB[call]
    return sorted({0, per - 1, per, per + 63, per + 64, total - 1} | set(range(0, total, (total // 12) | 1)))


def restate(call, slip, A, B, c, theta, cap=1000000, pairs=None, w_a=None, w_b=None, normalize=False):
    """one restatement on 5x4; with `pairs` (flat indices) the arrays lead with [len(pairs)] and the policy gradient's are the
    per-pair ones only"""
    lists, starts = pitch(slip)
    if call == "match":
        return mon.match_outcomes(lists, starts, A, B, c, theta, cap, pairs)
    if call == "occupancy":
        return ocn.occupancy(lists, starts, A, B, c, theta, cap, pairs, features_of(NS), in_lists(slip))
    assert call == "gradient"
    if pairs is None:
        return pgn.policy_gradient(lists, starts, A, B, c, theta, w_a, w_b, normalize, cap, in_lists(slip))
    flat = np.asarray(pairs)
    return pgn.pairs(lists, starts, A[flat // len(B)], B[flat % len(B)], c, theta, cap, in_lists(slip))


CALLS = ("match", "occupancy", "gradient")
_three = {}


def three_calls(name, slip, A, B, c, theta, cap=1000000):
    """{call: its restatement of A x B} with the policy gradient under weights(n) and normalize=True; computed once per
    (name, slip, c, theta, cap) — `name` stands for the policies"""
    key = (name, slip, c, theta, cap)
    if key not in _three:
        _three[key] = {call: restate(call, slip, A, B, c, theta, cap, w_a=weights(len(A)), w_b=weights(len(B)), normalize=True)
                       for call in CALLS}
    return _three[key]


def counts(r):
    """{"match", "occupancy", "V", "D"}: the sweep counts of three_calls' result"""
    return {"match": r["match"]["iterations"], "occupancy": r["occupancy"]["iterations"], "V": r["gradient"]["iterations"][..., 0],
            "D": r["gradient"]["iterations"][..., 1]}
