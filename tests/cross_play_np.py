"""The cross-play matrix of two sets of mixed policies (include/soccer_hip.h, "cross-play") restated in numpy: pair (i, j) is
best_response_np.evaluate on (pi_a[i], pi_b[j]) — every pair with its own stopping sweep — and payoff[i][j] is the sequential
sum of V[i][j] over the initial states in ISD order, from 0.0, divided by their number.  tests/test_gpu_cross_play.py holds the
device to it bit for bit; tests/test_cross_play_np.py checks what it computes where there is no GPU."""
import numpy as np

import best_response_np as brn


def isd_obs(orc):
    """the oracle's initial states as observation indices, in ISD order"""
    lut, kind, gv, isd, isdp = orc.tables()
    W, H = orc.W, orc.H
    return [int(lut[((((int(s[0]) * W + int(s[1])) * H + int(s[2])) * W + int(s[3])) << 1) | int(s[4])]) for s in isd]


def kickoff(V, starts):
    """[.., nS] -> [..]: the mean over the initial states, summed in their order from 0.0"""
    acc = np.zeros(V.shape[:-1])
    for s in starts:
        acc = acc + V[..., s]
    return acc / float(len(starts))


def cross_play(lists, starts, pi_a, pi_b, gamma, theta, max_sweeps=1000000):
    """pi_a [n_a, nS, 5], pi_b [n_b, nS, 5] -> (payoff[n_a, n_b], iterations[n_a, n_b], V[n_a, n_b, nS])"""
    pi_a = np.asarray(pi_a, np.float64); pi_b = np.asarray(pi_b, np.float64)
    pi_a = pi_a.reshape((-1,) + pi_a.shape[-2:]); pi_b = pi_b.reshape((-1,) + pi_b.shape[-2:])
    na, nb, nS = pi_a.shape[0], pi_b.shape[0], pi_a.shape[1]
    V, it = brn.evaluate(lists, np.repeat(pi_a, nb, axis=0), np.tile(pi_b, (na, 1, 1)), gamma, theta, max_sweeps)
    V = V.reshape(na, nb, nS)
    return kickoff(V, starts), it.reshape(na, nb), V
