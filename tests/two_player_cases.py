"""The cases of the two-player edge tests on 5x4 at slips 0.0 and 0.2 — the policies, the caps, the unusual and the refused
policy rows, the samples of pairs and the matrix that the library's own pass split is run on — with the restatements' lists
they are solved over.  No GPU is needed here: tests/test_two_player_edges_np.py shows on the restatements alone that each case
reaches its path, tests/test_gpu_two_player_edges.py holds the device to the restatements on the same inputs."""
import functools

import numpy as np

from oracle.oracle import Oracle

import best_response_np as brn
import cross_play_np as cpn
from minimax_q_np import shapley_lists

W, H, NS = 5, 4, 761
SLIPS = [0.0, 0.2]
THETA = 1e-10
INF = float("inf")
UNDISCOUNTED_CAP = 200                  # discount 1: the uniform policy's response stops at 111 / 159, Dirichlet(0.2)'s is still open
THETA0_CAPS = [15, 16, 17, 32, 33]      # theta = 0, either side of the 16 sweeps between two synchronisations
TIE_GAMMAS = [0.5, 0.9]
# slip 0: tied states per policy of edge_policies(), by (discount, player), as the restatement has them
TIE_COUNTS = {(0.5, 0): [60, 42, 268, 342], (0.5, 1): [60, 42, 261, 342], (0.9, 0): [54, 38, 293, 337], (0.9, 1): [54, 45, 263, 337]}
GAMMA0_TIED = 722                       # discount 0: live states whose optimum more than one action attains, of 760
ROW_TOL = 1e-8 + 1e-5                   # |sum - 1| a policy row may have (include/soccer_hip.h, opponent_policy's rule)
# the library's own pass split: 1024 x 87 = 89 088 pairs, above the 88 128 whose two V buffers stay under 1 GiB on 5x4.
# discount 0.05: |V_k - V_{k-1}| <= 0.05^(k-1) * max|V_1| <= 0.05^(k-1), below 1e-10 from k = 9 on, for every pair of policies
PASS_NA, PASS_NB, PASS_GAMMA, PASS_SWEEPS = 1024, 87, 0.05, 9
PASS_PAIRS = (2 ** 30 // (16 * NS)) // 64 * 64


@functools.lru_cache(maxsize=None)
def pitch(slip):
    """(the oracle's two-player lists, its initial states as observation indices), built once per slip"""
    orc = Oracle(W, H, slip, n=1, seed=0)
    assert orc.nS == NS
    return shapley_lists(orc), cpn.isd_obs(orc)


def edge_policies():
    """uniform, Dirichlet(0.2) rows, one-hot rows, 'always action 2': [4, nS, 5]"""
    rng = np.random.default_rng(41)
    return np.stack([np.full((NS, 5), 0.2), rng.dirichlet(np.full(5, 0.2), NS), brn.onehot(rng.integers(0, 5, NS)),
                     brn.onehot(np.full(NS, 2))])


def odd_rows():
    """two policies [2, nS, 5] of rows that are accepted but unusual, by state index mod 4: 0 a Dirichlet row, 1 zeros written
    as -0.0 (around one 1.0, or around two 0.5s), 2 subnormal entries next to ordinary ones, 3 a Dirichlet row scaled to sum
    to 1 + 9e-6 or 1 - 9e-6"""
    rng = np.random.default_rng(43)
    pol = rng.dirichlet(np.ones(5), (2, NS))
    for p in pol:
        for s in range(1, NS):
            if s % 4 == 1:
                row = np.full(5, -0.0)
                if s % 8 == 1:
                    row[rng.integers(0, 5)] = 1.0
                else:
                    row[rng.choice(5, 2, replace=False)] = 0.5
                p[s] = row
            elif s % 4 == 2:
                row = np.array([0.25, 0.25, 0.5, 5e-324, 1e-310])
                p[s] = row[rng.permutation(5)]
            elif s % 4 == 3:
                p[s] = p[s] * (1.0 + 9e-6 if s % 8 == 3 else 1.0 - 9e-6)
    return pol


def refused_rows():
    """(row, the message's words): rows the rule refuses"""
    base = np.full(5, 0.2)
    return [(base * (1.0 + 1.2e-5), "does not sum to 1"), (base * (1.0 - 1.2e-5), "does not sum to 1"),
            (np.array([0.2, 0.2, INF, 0.2, 0.2]), "does not sum to 1")]


def row_accepted(row):
    """the documented rule: every entry >= 0 (a NaN is not), and the sequential sum within ROW_TOL of 1"""
    total = 0.0
    for p in row.tolist():
        if not p >= 0.0:
            return False
        total = total + p
    return bool(abs(total - 1.0) <= ROW_TOL)


def tied_states(Qr, player):
    """per policy, the live states whose optimum (B's minimum for player 0, A's maximum for player 1) several actions attain"""
    best = Qr.min(-1) if player == 0 else Qr.max(-1)
    return ((Qr == best[..., None]).sum(-1) > 1)[:, 1:].sum(1)


def boundary_sample(total, step=64):
    """the first and the last pair and the pairs either side of each multiple of `step`"""
    return sorted({0, total - 1} | {m - 1 for m in range(step, total, step)} | set(range(step, total, step)))


def pass_policies():
    """(pi_a [1024, nS, 5], pi_b [87, nS, 5]) for the pass split: uniform, Dirichlet(1), Dirichlet(0.2) and one-hot rows in turn"""
    rng = np.random.default_rng(47)
    kinds = [lambda: np.full((NS, 5), 0.2), lambda: rng.dirichlet(np.ones(5), NS), lambda: rng.dirichlet(np.full(5, 0.2), NS),
             lambda: brn.onehot(rng.integers(0, 5, NS))]
    return np.stack([kinds[k % 4]() for k in range(PASS_NA)]), np.stack([kinds[(k + 1) % 4]() for k in range(PASS_NB)])


def pass_sample():
    """pairs of the 1024 x 87 matrix, as flat indices: the first, the two either side of the pass boundary, the last pair of
    the ragged second pass and its first full wave's ends, and 33 more spread over the matrix at an odd stride"""
    total = PASS_NA * PASS_NB
    return sorted({0, PASS_PAIRS - 1, PASS_PAIRS, PASS_PAIRS + 63, PASS_PAIRS + 64, total - 1} | set(range(0, total, 2783)))


def in_chunks(solve, *policies, chunk=32):
    """a restatement's solve of a large batch, 32 members at a time: every member's arithmetic is its own, so the bits are
    those of one call, and the temporaries stay in the cache (256 members: half the time)"""
    parts = [solve(*[p[i:i + chunk] for p in policies]) for i in range(0, len(policies[0]), chunk)]
    return [np.concatenate(x) for x in zip(*parts)]


def restated_pairs(slip, A, B, flat, gamma, theta, max_sweeps=1000000):
    """(payoff, iterations, V) of the pairs `flat` (indices into the row-major n_a x n_b matrix), by the restatement"""
    lists, starts = pitch(slip)
    flat = np.asarray(flat)
    V, it = brn.evaluate(lists, A[flat // len(B)], B[flat % len(B)], gamma, theta, max_sweeps)
    return cpn.kickoff(V, starts), it, V
