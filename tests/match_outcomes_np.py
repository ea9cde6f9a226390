"""Match outcomes of two sets of mixed policies (include/soccer_hip.h, "match outcomes") restated in numpy over the two-player
lists of minimax_q_np.shapley_lists: per pair the three value vectors W_A (A scores the goal that ends the game), W_B (B does)
and L (the steps the game lasts) when every step is followed by another with probability c.  The definition's float64
arithmetic, every sum sequential from 0.0 in index order; the three channels sit on the last axis, so one gather of V[next]
serves all three.  tests/test_gpu_match_outcomes.py holds the device to it bit for bit; tests/test_match_outcomes_np.py
checks what it computes where there is no GPU, and that each channel is best_response_np's evaluation with another reward."""
import numpy as np

import best_response_np as brn
from cross_play_np import kickoff

CHANNELS = ("win_a", "win_b", "length")
CHUNK = 4           # pairs swept together: every pair's arithmetic is its own, and the temporaries stay in the cache


def channel_lists(lists):
    """the lists with list position first and the three channels' rewards last: prob[K, nS, 25, 1], next[K, nS, 25],
    (reward > 0, reward < 0, 1.0)[K, nS, 25, 3], (not done)[K, nS, 25, 1]"""
    Pp, Pn, Pr, Pd = lists
    # what the indicators rest on: a reward is -1, 0 or +1, and nonzero only on an entry that ends the game
    assert np.isin(Pr, (-1.0, 0.0, 1.0)).all(), "a reward that is not -1, 0 or +1"
    assert (Pd[Pr != 0.0] == 0.0).all(), "a reward on an entry that does not end the game"
    ind = np.stack([Pr > 0, Pr < 0, np.ones(Pr.shape, bool)], -1).astype(np.float64)
    first = lambda a: np.ascontiguousarray(np.moveaxis(a, 2, 0))        # noqa: E731
    # (c * F[next]) * (not done) is c * F[next] where the entry goes on and +0.0 where it ends the game, and +0.0 is what
    # c * F[0] is in every sweep (row 0 of a policy counts as zeros): an entry that ends the game reads state 0 instead
    return first(Pp)[..., None], first(np.where(Pd != 0.0, Pn, 0)), first(ind)


def sweep(chans, x, y, F, c):
    """one sweep of every pair: F_k[P, nS, 3] from F_{k-1}; x, y are [P, nS, 5]"""
    prob, nxt, ind = chans
    P, nS = F.shape[:2]
    assert (F[:, 0] == 0).all() and not np.signbit(F[:, 0]).any()
    cF = c * F
    q = np.zeros((P, nS, 25, 3))
    for k in range(prob.shape[0]):                                      # q = q + prob * (ind + (c * F[next]) * (not done))
        t = cF[:, nxt[k]]
        t += ind[k]; t *= prob[k]
        q += t
    Q = q.reshape(P, nS, 5, 5, 3)
    inner = np.zeros((P, nS, 5, 3))
    for b in range(5):
        inner = inner + y[:, :, None, b, None] * Q[:, :, :, b]
    v = np.zeros((P, nS, 3))
    for a in range(5):
        v = v + x[:, :, a, None] * inner[:, :, a]
    return v


def solve(lists, x, y, c, theta, max_sweeps=1000000):
    """x, y: [P, nS, 5], pair p is (x[p], y[p]).  Every pair stops at its own first k with max over the three channels and
    all states of |F_k - F_{k-1}| < theta and keeps that sweep's vectors.  Returns (F[P, 3, nS], iterations[P]); iterations ==
    max_sweeps where a pair did not get there."""
    chans = channel_lists(lists)
    x = brn._policies(x); y = brn._policies(y)                          # row 0 is not read: it counts as zeros
    P, nS = x.shape[:2]
    F = np.zeros((P, nS, 3))
    it = np.full(P, int(max_sweeps), np.int64)
    for p0 in range(0, P, CHUNK):
        live = np.arange(p0, min(p0 + CHUNK, P))
        for k in range(1, int(max_sweeps) + 1):
            f = sweep(chans, x[live], y[live], F[live], c)
            d = np.abs(f - F[live]).max((1, 2))
            F[live] = f
            it[live[d < theta]] = k
            live = live[~(d < theta)]
            if live.size == 0:
                break
    return np.ascontiguousarray(np.moveaxis(F, 2, 1)), it


def match_outcomes(lists, starts, pi_a, pi_b, c, theta, max_sweeps=1000000, pairs=None):
    """pi_a [n_a, nS, 5], pi_b [n_b, nS, 5] -> a dict of win_a, win_b, length, iterations [n_a, n_b] and values
    [n_a, n_b, 3, nS].  pairs: flat indices i * n_b + j to solve instead of all of them; the arrays are then [len(pairs), ..]."""
    pi_a = np.asarray(pi_a, np.float64); pi_b = np.asarray(pi_b, np.float64)
    pi_a = pi_a.reshape((-1,) + pi_a.shape[-2:]); pi_b = pi_b.reshape((-1,) + pi_b.shape[-2:])
    na, nb, nS = pi_a.shape[0], pi_b.shape[0], pi_a.shape[1]
    flat = np.arange(na * nb) if pairs is None else np.asarray(pairs, np.int64)
    F, it = solve(lists, pi_a[flat // nb], pi_b[flat % nb], c, theta, max_sweeps)
    shape = (na, nb) if pairs is None else (flat.size,)
    out = {name: kickoff(F[:, ch], starts).reshape(shape) for ch, name in enumerate(CHANNELS)}
    out["iterations"] = it.reshape(shape)
    out["values"] = F.reshape(shape + (3, nS))
    return out
