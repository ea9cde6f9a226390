"""State occupancy of two sets of mixed policies (include/soccer_hip.h, "state occupancy") restated in numpy over the two-player
lists of minimax_q_np.shapley_lists: per pair the expected number of visits D[s] to every state from kick-off when every step
is followed by another with probability c.  The definition's float64 arithmetic: D_k[s'] = mu[s'] + the sequential sum, in
in-list order from 0.0, of prob * ((x[s][a] * y[s][b]) * (c * D_{k-1}[s])).  The in-lists are built here too (in_lists), the
way csrc/soccer_inlists.hpp builds them.  tests/test_gpu_occupancy.py holds the device to it bit for bit;
tests/test_occupancy_np.py checks what it computes where there is no GPU."""
import numpy as np

import best_response_np as brn

PAD = 4             # kPlanPad
CHUNK = 4           # pairs swept together: every pair's arithmetic is its own, and the temporaries stay in the cache


def in_lists(n_states, key, prob, nxt, done):
    """The in-lists of out-entries given in walk order (ascending key, then position inside the key's list): key, prob,
    next state and done bit per entry.  An entry is kept if its done bit is clear and its source state key // 25 is not 0.
    Returns (in_offset[n_states + 1], in_prob, in_key): the in-list of s' is in_offset[s'] .. in_offset[s' + 1], its kept
    entries in walk order, padded to a multiple of PAD with (0.0, 0)."""
    key = np.asarray(key, np.int64); prob = np.asarray(prob, np.float64); nxt = np.asarray(nxt, np.int64)
    keep = np.flatnonzero((np.asarray(done) == 0) & (key >= 25))
    assert (np.diff(key) >= 0).all(), "the entries are not in walk order"
    assert ((nxt[keep] >= 0) & (nxt[keep] < n_states)).all()
    order = keep[np.argsort(nxt[keep], kind="stable")]                  # by next state, walk order kept inside each
    count = np.bincount(nxt[keep], minlength=n_states)
    padded = (count + PAD - 1) // PAD * PAD
    off = np.concatenate([[0], np.cumsum(padded)]).astype(np.int64)
    in_prob = np.zeros(off[-1]); in_key = np.zeros(off[-1], np.int64)
    start = np.concatenate([[0], np.cumsum(count)])[:-1]
    slot = off[nxt[order]] + (np.arange(order.size) - start[nxt[order]])
    in_prob[slot] = prob[order]; in_key[slot] = key[order]
    return off, in_prob, in_key


def in_lists_of(lists):
    """in_lists of shapley_lists' padded arrays [nS, 25, K] (their padding has prob 0, next 0 and 1 - done = 0: dropped as done)"""
    Pp, Pn, Pr, Pd = lists
    nS, _, K = Pp.shape
    key = np.repeat(np.arange(nS * 25), K)
    return in_lists(nS, key, Pp.reshape(-1), Pn.reshape(-1), (Pd.reshape(-1) == 0.0))


def levels_of(inl, n_states):
    """the in-lists by position, for sweeps without a loop over states: (order, cuts, prob, key) where order lists the states by
    descending in-list length, and entries cuts[t] .. cuts[t + 1] of prob / key are the t-th in-entries of the states
    order[:cuts[t + 1] - cuts[t]] (those whose in-list is longer than t)"""
    off, in_prob, in_key = inl
    size = np.diff(off)
    order = np.argsort(-size, kind="stable")
    at, cuts = [], [0]
    for t in range(int(size.max()) if size.size else 0):
        st = order[:int((size > t).sum())]
        at.append(off[st] + t)
        cuts.append(cuts[-1] + st.size)
    at = np.concatenate(at) if at else np.zeros(0, np.int64)
    return order, cuts, in_prob[at], in_key[at]


def start_distribution(n_states, starts):
    mu = np.zeros(n_states)
    assert len(set(starts)) == len(starts)
    mu[list(starts)] = 1.0 / float(len(starts))
    return mu


def solve(lists, starts, x, y, c, theta, max_sweeps=1000000, inl=None):
    """x, y: [P, nS, 5], pair p is (x[p], y[p]).  Every pair stops at its own first k with max_s |D_k[s] - D_{k-1}[s]| < theta
    and keeps that sweep's vector.  Returns (D[P, nS], iterations[P]); iterations == max_sweeps where a pair did not get there."""
    x = brn._policies(x); y = brn._policies(y)                          # row 0 is not read: it counts as zeros
    P, nS = x.shape[:2]
    order, cuts, prob, key = levels_of(in_lists_of(lists) if inl is None else inl, nS)
    mu = start_distribution(nS, starts)[order, None]
    xf = x.reshape(P, nS * 5); yf = y.reshape(P, nS * 5)
    src = key // 25
    D = np.zeros((P, nS))
    it = np.full(P, int(max_sweeps), np.int64)
    for p0 in range(0, P, CHUNK):
        own = np.arange(p0, min(p0 + CHUNK, P))
        # x[s][a] * y[s][b] of every in-entry, [entries, pairs]: the same product in every sweep
        w_all = np.ascontiguousarray((xf[own][:, key // 5] * yf[own][:, src * 5 + key % 5]).T)
        live, w = np.arange(own.size), w_all
        for k in range(1, int(max_sweeps) + 1):
            old = D[own[live]]
            t = np.ascontiguousarray((c * old).T)[src]                  # c * D_{k-1}[s] of every in-entry
            t *= w; t *= prob[:, None]                                  # prob * ((x * y) * (c * D[s]))
            acc = np.zeros((nS, live.size))                             # rows in `order`: the states with a t-th entry lead
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                acc[:hi - lo] += t[lo:hi]
            new = np.zeros((live.size, nS))
            new[:, order] = (mu + acc).T
            new[:, 0] = 0.0                                             # D[0] is 0.0 in every sweep
            d = np.abs(new - old).max(1)
            D[own[live]] = new
            it[own[live[d < theta]]] = k
            if (d < theta).any():
                live = live[~(d < theta)]
                w = np.ascontiguousarray(w_all[:, live])
            if live.size == 0:
                break
    return D, it


def sequential_sum(a):
    """[.., n] -> [..]: the sum over the last axis in index order from 0.0"""
    return np.add.accumulate(np.concatenate([np.zeros(a.shape[:-1] + (1,)), a], -1), axis=-1)[..., -1]


def occupancy(lists, starts, pi_a, pi_b, c, theta, max_sweeps=1000000, pairs=None, features=None, inl=None):
    """pi_a [n_a, nS, 5], pi_b [n_b, nS, 5] -> a dict of length, iterations [n_a, n_b], expect [n_a, n_b, n_f] and occupancy
    [n_a, n_b, nS].  pairs: flat indices i * n_b + j to solve instead of all of them; the arrays are then [len(pairs), ..]."""
    pi_a = np.asarray(pi_a, np.float64); pi_b = np.asarray(pi_b, np.float64)
    pi_a = pi_a.reshape((-1,) + pi_a.shape[-2:]); pi_b = pi_b.reshape((-1,) + pi_b.shape[-2:])
    na, nb, nS = pi_a.shape[0], pi_b.shape[0], pi_a.shape[1]
    flat = np.arange(na * nb) if pairs is None else np.asarray(pairs, np.int64)
    D, it = solve(lists, starts, pi_a[flat // nb], pi_b[flat % nb], c, theta, max_sweeps, inl)
    shape = (na, nb) if pairs is None else (flat.size,)
    F = np.zeros((0, nS)) if features is None else np.asarray(features, np.float64).reshape(-1, nS)
    expect = np.stack([sequential_sum(D * f) for f in F], -1) if F.shape[0] else np.zeros((flat.size, 0))
    return {"length": sequential_sum(D).reshape(shape), "expect": expect.reshape(shape + (F.shape[0],)),
            "iterations": it.reshape(shape), "occupancy": D.reshape(shape + (nS,))}


def mean_reward(lists, x, y):
    """r(s) = sum_ab x[s][a] * y[s][b] * sum prob * reward of one pair, [nS] (for the cross-checks; its rounding is not pinned)"""
    Pp, Pn, Pr, Pd = lists
    nS = Pp.shape[0]
    x = brn._policies(x)[0]; y = brn._policies(y)[0]
    return ((x[:, :, None] * y[:, None, :]).reshape(nS, 25) * (Pp * Pr).sum(2)).sum(1)
