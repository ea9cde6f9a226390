"""Exact policy gradients of two sets of mixed policies and gradient play on them (include/soccer_hip.h, "exact policy
gradients") restated in numpy.  Composed of what the other restatements define: per pair V is best_response_np.evaluate, D is
occupancy_np.solve with the discount as the continuation probability, q is best_response_np.list_q from the pair's final V, Q_a
and Q_b are mixed_cols and mixed_rows of it.  Added here: the weighted sums over the other side's policies in ascending order
from 0.0, the normalisation by the reach, the projection onto the simplex and the step of gradient play.
tests/test_gpu_policy_gradient.py holds the device to it bit for bit; tests/test_policy_gradient_np.py checks what it computes
where there is no GPU."""
import numpy as np

import best_response_np as brn
import cross_play_np as cpn
import occupancy_np as ocn


def pairs(lists, starts, x, y, gamma, theta, max_sweeps=1000000, inl=None):
    """x, y: [P, nS, 5], pair p is (x[p], y[p]).  A dict of per-pair arrays: V, occupancy [P, nS], q_a, q_b [P, nS, 5], payoff
    [P] and iterations [P, 2] = (k_V, k_D); a solve that is open at max_sweeps holds its last iterate."""
    V, kV = brn.evaluate(lists, x, y, gamma, theta, max_sweeps)
    D, kD = ocn.solve(lists, starts, x, y, gamma, theta, max_sweeps, inl)
    x0 = brn._policies(x); y0 = brn._policies(y)                        # row 0 counts as zeros
    Q = brn.list_q(lists, V, gamma)                                     # one more backup from the final V
    return {"V": V, "occupancy": D, "q_a": brn.mixed_cols(y0, Q), "q_b": brn.mixed_rows(x0, Q), "payoff": cpn.kickoff(V, starts),
            "iterations": np.stack([kV, kD], -1)}


def weights_of(w, n):
    return np.full(n, 1.0 / float(n)) if w is None else np.asarray(w, np.float64)


def weighted_sum(w, terms):
    """sum_k w[k] * terms[k] over ascending k from 0.0 (the leading axis)"""
    acc = np.zeros(terms.shape[1:])
    for k in range(terms.shape[0]):
        acc = acc + w[k] * terms[k]
    return acc


def normalized(grad, reach):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(reach[..., None] > 0.0, grad / reach[..., None], 0.0)


def reduce(D, q_a, q_b, w_a=None, w_b=None, normalize=False):
    """D [n_a, n_b, nS], q_a, q_b [n_a, n_b, nS, 5] -> (grad_a [n_a, nS, 5], grad_b [n_b, nS, 5], reach_a [n_a, nS], reach_b
    [n_b, nS]): player A's sums run over ascending j with w_b, player B's over ascending i with w_a"""
    na, nb = D.shape[:2]
    w_a, w_b = weights_of(w_a, na), weights_of(w_b, nb)
    DQa = D[..., None] * q_a; DQb = D[..., None] * q_b
    reach_a = np.stack([weighted_sum(w_b, D[i]) for i in range(na)])
    grad_a = np.stack([weighted_sum(w_b, DQa[i]) for i in range(na)])
    reach_b = np.stack([weighted_sum(w_a, D[:, j]) for j in range(nb)])
    grad_b = np.stack([weighted_sum(w_a, DQb[:, j]) for j in range(nb)])
    if normalize:
        grad_a, grad_b = normalized(grad_a, reach_a), normalized(grad_b, reach_b)
    return grad_a, grad_b, reach_a, reach_b


def policy_gradient(lists, starts, pi_a, pi_b, gamma, theta, w_a=None, w_b=None, normalize=False, max_sweeps=1000000, inl=None):
    """pi_a [n_a, nS, 5], pi_b [n_b, nS, 5] -> the device's dict: payoff, grad_a, grad_b, reach_a, reach_b, q_a, q_b, V,
    occupancy and iterations [n_a, n_b, 2]"""
    pi_a = np.asarray(pi_a, np.float64); pi_b = np.asarray(pi_b, np.float64)
    pi_a = pi_a.reshape((-1,) + pi_a.shape[-2:]); pi_b = pi_b.reshape((-1,) + pi_b.shape[-2:])
    na, nb = pi_a.shape[0], pi_b.shape[0]
    r = pairs(lists, starts, np.repeat(pi_a, nb, axis=0), np.tile(pi_b, (na, 1, 1)), gamma, theta, max_sweeps, inl)
    out = {k: v.reshape((na, nb) + v.shape[1:]) for k, v in r.items()}
    out["grad_a"], out["grad_b"], out["reach_a"], out["reach_b"] = reduce(out["occupancy"], out["q_a"], out["q_b"], w_a, w_b, normalize)
    return out


def project(v):
    """[.., 5] -> [.., 5]: the projection onto the simplex, csrc/soccer_simplex.hpp's definition"""
    v = np.asarray(v, np.float64)
    u = -np.sort(-v, axis=-1)                                           # descending
    css = np.zeros(v.shape[:-1])
    tau = None
    for k in range(5):
        css = css + u[..., k]
        t = (css - 1.0) / float(k + 1)
        tau = t if k == 0 else np.where(u[..., k] - t > 0.0, t, tau)
    d = v - tau[..., None]
    return np.where(d > 0.0, d, 0.0)


def step(x, y, g_a, g_b, prev_a, prev_b, first, eta_a, eta_b, optimism):
    """one update of gradient play: (x', y', prev_a', prev_b').  Row 0 of a policy is never touched, and a side whose eta is
    0.0 is held fixed: none of its rows is projected."""
    if first:
        prev_a, prev_b = g_a, g_b
    d_a = g_a + optimism * (g_a - prev_a)
    d_b = g_b + optimism * (g_b - prev_b)
    x2 = np.array(x, np.float64); y2 = np.array(y, np.float64)
    if eta_a != 0.0:
        x2[:, 1:] = project(x[:, 1:] + eta_a * d_a[:, 1:])
    if eta_b != 0.0:
        y2[:, 1:] = project(y[:, 1:] - eta_b * d_b[:, 1:])
    return x2, y2, g_a, g_b


def gradient_play(lists, starts, x, y, n_steps, gamma, theta, eta_a, eta_b, optimism=0.0, normalize=False, w_a=None, w_b=None,
                  max_sweeps=1000000, inl=None):
    """n_steps of gradient play from (x [n_a, nS, 5], y [n_b, nS, 5]): (x, y, prev_a, prev_b, trace [n_steps, n_a, n_b])"""
    x = np.array(x, np.float64); y = np.array(y, np.float64)
    prev_a = np.zeros(x.shape); prev_b = np.zeros(y.shape)
    trace = []
    for t in range(n_steps):
        r = policy_gradient(lists, starts, x, y, gamma, theta, w_a, w_b, normalize, max_sweeps, inl)
        trace.append(r["payoff"])
        x, y, prev_a, prev_b = step(x, y, r["grad_a"], r["grad_b"], prev_a, prev_b, t == 0, eta_a, eta_b, optimism)
    return x, y, prev_a, prev_b, np.stack(trace) if trace else np.zeros((0, x.shape[0], y.shape[0]))
