"""The single-agent planners (include/soccer_hip.h, "planners"; planner_kernel in csrc/soccer_planner_kernels.hpp) restated in
numpy over the CPU oracle's single_agent_lists: the kernel's float64 arithmetic, every sum sequential from 0.0 in the kernel's
order, vectorised over the states so that it runs on pitches where the oracle's Python loops do not.
tests/test_gpu_planner_shapes.py holds the device to it bit for bit; tests/test_planners_np.py pins it to the oracle's loops
and to the reference's fixtures where there is no GPU.

Every planner takes max_sweeps, counts sweeps the way the kernel's `sweeps` does (policy iteration and modified policy
iteration: the total over all their evaluations) and returns a Plan whose `capped` says that the cap was reached before the
stopping rule; the arrays are then what the kernel leaves in its outputs (see each function)."""
from collections import namedtuple

import numpy as np

Plan = namedtuple("Plan", "pi V Q counter sweeps capped")      # counter: what the C call returns in *iterations / *sweeps


def from_oracle(orc, learner, policy):
    """(lists, rows) of a single-agent game: the padded lists of the list family and the sparse rows of the dense one"""
    from oracle.oracle import single_agent_lists
    P = single_agent_lists(orc, learner, policy)
    n_goal = int(np.count_nonzero(orc.tables()[1] == 2))
    lists = pad_lists(P, orc.nS)
    return lists, sparse_rows(P, orc.nS, n_goal, lists)


# ---- the list family: value iteration, policy evaluation / improvement / iteration ----------------------------------------
def pad_lists(P, nS):
    """oracle.single_agent_lists' P[s][a] -> (prob, next, reward, notdone), each [nS, 5, K]; a padding entry has prob 0,
    reward 0 and done set (it adds +0.0)"""
    K = max(len(P[s][a]) for s in range(nS) for a in range(5))
    Pp = np.zeros((nS, 5, K)); Pn = np.zeros((nS, 5, K), np.int64); Pr = np.zeros((nS, 5, K)); Pnd = np.zeros((nS, 5, K))
    for s in range(nS):
        for a in range(5):
            for k, (p, ns, r, done) in enumerate(P[s][a]):
                Pp[s, a, k] = p; Pn[s, a, k] = ns; Pr[s, a, k] = r; Pnd[s, a, k] = 0.0 if done else 1.0
    return Pp, Pn, Pr, Pnd


def list_q(lists, V, gamma):
    """Q[s, a] = sum_k prob * (reward + (gamma * V[next]) * (not done)) in list order"""
    Pp, Pn, Pr, Pnd = lists
    q = np.zeros(Pp.shape[:2])
    for k in range(Pp.shape[2]):
        q = q + Pp[..., k] * (Pr[..., k] + (gamma * V[Pn[..., k]]) * Pnd[..., k])
    return q


def _greedy(Q):
    pi = Q.argmax(1)                                            # the first maximum
    return pi, Q[np.arange(Q.shape[0]), pi]


def value_iteration(lists, theta, gamma, max_sweeps=1000000):
    """V is the iterate the last sweep started from (the reference returns the pre-update V), Q and pi that sweep's; at the
    cap the same three of the last sweep run."""
    V = np.zeros(lists[0].shape[0])
    sweeps = 0
    while True:
        Q = list_q(lists, V, gamma)
        pi, newV = _greedy(Q)
        delta = np.abs(V - newV).max()
        sweeps += 1
        if delta < theta:
            return Plan(pi, V, Q, sweeps, sweeps, False)
        if sweeps >= max_sweeps:
            return Plan(pi, V, Q, sweeps, sweeps, True)
        V = newV


def _evaluate(lists, pi, theta, gamma, max_sweeps, sweeps):
    """policy evaluation from zeros; `sweeps` is the count so far -> (the last iterate computed, sweeps, capped)"""
    Pp, Pn, Pr, Pnd = (x[np.arange(x.shape[0]), pi] for x in lists)                 # [nS, K]: the rows of pi
    prev = np.zeros(Pp.shape[0])
    while True:
        V = np.zeros(Pp.shape[0])
        for k in range(Pp.shape[1]):
            V = V + Pp[:, k] * (Pr[:, k] + (gamma * prev[Pn[:, k]]) * Pnd[:, k])
        delta = np.abs(prev - V).max()
        sweeps += 1
        if delta < theta:
            return V, sweeps, False
        if sweeps >= max_sweeps:
            return V, sweeps, True
        prev = V


def policy_evaluation(lists, pi, theta, gamma, max_sweeps=1000000):
    """V is the last iterate computed, also at the cap"""
    V, sweeps, capped = _evaluate(lists, np.asarray(pi, np.int64), theta, gamma, max_sweeps, 0)
    return Plan(None, V, None, sweeps, sweeps, capped)


def policy_improvement(lists, V, gamma):
    Q = list_q(lists, np.asarray(V, np.float64), gamma)
    return Plan(Q.argmax(1), None, Q, 1, 0, False)


def policy_iteration(lists, pi0, theta, gamma, max_sweeps=1000000):
    """counter: improvements made.  At the cap: V is the iterate at which the evaluation in progress was cut off, Q and pi one
    improvement from that V (the kernel still makes it), counted."""
    pi = np.asarray(pi0, np.int64)
    sweeps = outer = 0
    while True:
        V, sweeps, capped = _evaluate(lists, pi, theta, gamma, max_sweeps, sweeps)
        Q = list_q(lists, V, gamma)
        new_pi = Q.argmax(1)
        outer += 1
        changed = bool(np.any(new_pi != pi))
        pi = new_pi
        if not changed or capped:
            return Plan(pi, V, Q, outer, sweeps, capped)


# ---- the dense family: policy_eval_dense, modified_policy_iteration, on sparse rows of Pmat ------------------------------
def sparse_rows(P, nS, n_goal, lists=None):
    """Pmat[s, :, a] and Rmat[s, a] as oracle.single_agent_mats accumulates them (Rmat[s][a] = 0, then += p * r;
    Pmat[s][ns][a] += p, in tuple and entry order), kept as the touched next states of every (s, a) in ascending order with
    exact zeros dropped: (prob[nS, 5, K], next[nS, 5, K], Rmat[nS, 5]); a padding entry is (0.0, 0).  A live observation
    index has one tuple, whose lists are P[s]; index 0 collects the n_goal goal tuples, whose lists are all P[0], and its
    Rmat is the last one's."""
    Pp, Pn, Pr, _ = lists if lists is not None else pad_lists(P, nS)
    K = Pp.shape[2]
    Rm = np.zeros((nS, 5))
    for k in range(K):
        Rm = Rm + Pp[..., k] * Pr[..., k]
    key = np.where(Pp != 0.0, Pn, nS)                           # padding sorts last
    order = np.argsort(key, axis=-1, kind="stable")             # equal next states stay in entry order
    key = np.take_along_axis(key, order, -1); p = np.take_along_axis(Pp, order, -1)
    run = np.zeros((nS, 5, K))                                  # the running sum of the entry's segment
    acc = np.zeros((nS, 5))
    for k in range(K):
        first = key[..., k] != key[..., k - 1] if k else np.ones((nS, 5), bool)
        acc = np.where(first, 0.0, acc) + p[..., k]
        run[..., k] = acc
    last = np.ones((nS, 5, K), bool)
    last[..., :-1] = key[..., 1:] != key[..., :-1]
    keep = last & (key < nS) & (run != 0.0)
    # index 0: every goal tuple's entries, one after the other
    row0 = []
    for a in range(5):
        d = {}
        for _ in range(n_goal):
            for prob, ns, _r, _d in P[0][a]:
                d[ns] = d.get(ns, 0.0) + prob
        row0.append(sorted((ns, v) for ns, v in d.items() if v != 0.0))
    Km = max(int(keep.sum(-1).max()), max(len(r) for r in row0))
    left = np.argsort(~keep, axis=-1, kind="stable")[..., :Km]  # the kept entries first, in order
    kept = np.take_along_axis(keep, left, -1)
    Mp = np.where(kept, np.take_along_axis(run, left, -1), 0.0)
    Mn = np.where(kept, np.take_along_axis(key, left, -1), 0)
    Mp[0] = 0.0; Mn[0] = 0
    for a in range(5):
        for j, (ns, v) in enumerate(row0[a]):
            Mp[0, a, j] = v; Mn[0, a, j] = ns
    return Mp, Mn, Rm


def densify(rows):
    """(Pmat[nS, nS, 5], Rmat) of sparse_rows' output"""
    Mp, Mn, Rm = rows
    nS = Mp.shape[0]
    Pmat = np.zeros((nS, nS, 5))
    s, a, k = np.nonzero(Mp)
    Pmat[s, Mn[s, a, k], a] = Mp[s, a, k]
    return Pmat, Rm


def dense_dot(rows, v):
    """[nS, 5]: dot(Pmat[s, :, a], v), a sequential sum over the kept entries in ascending next state"""
    Mp, Mn, _ = rows
    acc = np.zeros(Mp.shape[:2])
    for k in range(Mp.shape[2]):
        acc = acc + Mp[..., k] * v[Mn[..., k]]
    return acc


def policy_eval_dense(rows, policy, theta, gamma, k=10000000, init=None, max_sweeps=10000000):
    """at most k sweeps of the stochastic policy[nS, 5] from init (zeros if None); V is the last iterate, also at the cap.
    Like the kernel, a sweep that reaches max_sweeps without meeting theta counts as capped even if it is the k-th."""
    policy = np.asarray(policy, np.float64)
    Rm = rows[2]
    v = np.zeros(Rm.shape[0]) if init is None else np.array(init, np.float64)
    sweeps, capped = 0, False
    for _ in range(int(k)):
        acc = dense_dot(rows, v)
        r_pi = np.zeros(v.shape); p_pi = np.zeros(v.shape)
        for a in range(5):
            r_pi = r_pi + policy[:, a] * Rm[:, a]
            p_pi = p_pi + acc[:, a] * policy[:, a]
        new = r_pi + gamma * p_pi
        delta = np.abs(new - v).max()
        v = new
        sweeps += 1
        if delta < theta:
            break
        if sweeps >= max_sweeps:
            capped = True
            break
    return Plan(None, v, None, sweeps, sweeps, capped)


def modified_policy_iteration(rows, k, theta, gamma, max_sweeps=10000000):
    """counter: evaluations made; a greedy step and every evaluation sweep count towards max_sweeps.  Converged, or capped at
    a greedy step: V = max_a Q of that step, pi its first argmax.  Capped inside an evaluation: V is that evaluation's last
    iterate, Q and pi the greedy step's that it started from, and the evaluation is counted."""
    Mp, Mn, Rm = rows
    nS = Rm.shape[0]
    v = np.zeros(nS)
    threshold = (theta * (1 - gamma)) / (2 * gamma)
    sweeps = outer = 0
    while True:
        Q = Rm + gamma * dense_dot(rows, v)
        pi, greedy_v = _greedy(Q)
        gap = np.abs(v - greedy_v).max()
        sweeps += 1
        if gap <= threshold:
            return Plan(pi, greedy_v, Q, outer, sweeps, False)
        if sweeps >= max_sweeps:
            return Plan(pi, greedy_v, Q, outer, sweeps, True)
        v = greedy_v
        idx = np.arange(nS)
        Ep, En, Er = Mp[idx, pi], Mn[idx, pi], Rm[idx, pi]
        capped = False
        for _ in range(int(k)):
            acc = np.zeros(nS)
            for j in range(Ep.shape[1]):
                acc = acc + Ep[:, j] * v[En[:, j]]
            new = Er + gamma * acc
            delta = np.abs(new - v).max()
            v = new
            sweeps += 1
            if delta < theta:
                break
            if sweeps >= max_sweeps:
                capped = True
                break
        outer += 1
        if capped:
            return Plan(pi, v, Q, outer, sweeps, True)
