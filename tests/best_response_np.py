"""Best responses to mixed policies and the value of a pair of them (include/soccer_hip.h, "best responses") restated in
numpy over the two-player lists of minimax_q_np.shapley_lists (the CPU oracle's transition relation): the definition's
float64 arithmetic, every sum sequential from 0.0 in index order.  tests/test_gpu_best_response.py holds the device to it
bit for bit; tests/test_best_response_np.py checks what it computes where there is no GPU."""
import numpy as np

RESPOND_B, RESPOND_A, EVAL_PAIR = 0, 1, 2


def list_q(lists, V, gamma):
    """Q[.., s, a, b] = sum_k prob * (reward + (gamma * V[.., next]) * (not done)) in list order; V is [.., nS]"""
    Pp, Pn, Pr, Pd = lists
    q = np.zeros(V.shape[:-1] + Pp.shape[:2])
    for k in range(Pp.shape[2]):
        q = q + Pp[:, :, k] * (Pr[:, :, k] + (gamma * V[..., Pn[:, :, k]]) * Pd[:, :, k])
    return q.reshape(q.shape[:-1] + (5, 5))


def mixed_rows(x, Q):
    """[.., b] = sum_a x[.., a] * Q[.., a, b], a = 0..4 in order"""
    acc = np.zeros(Q.shape[:-2] + (5,))
    for a in range(5):
        acc = acc + x[..., a, None] * Q[..., a, :]
    return acc


def mixed_cols(y, Q):
    """[.., a] = sum_b y[.., b] * Q[.., a, b], b = 0..4 in order"""
    acc = np.zeros(Q.shape[:-2] + (5,))
    for b in range(5):
        acc = acc + y[..., None, b] * Q[..., :, b]
    return acc


def sweep(lists, mode, x, y, V, gamma):
    """one sweep of every policy: (V_k, Qr_k, br_k) from V_{k-1}"""
    Q = list_q(lists, V, gamma)
    if mode == EVAL_PAIR:
        inner = mixed_cols(y, Q)
        v = np.zeros(V.shape)
        for a in range(5):
            v = v + x[..., a] * inner[..., a]
        return v, None, None
    Qr = mixed_rows(x, Q) if mode == RESPOND_B else mixed_cols(y, Q)
    br = Qr.argmin(-1) if mode == RESPOND_B else Qr.argmax(-1)          # the first index that attains it
    return np.take_along_axis(Qr, br[..., None], -1)[..., 0], Qr, br


def _policies(p):
    p = np.array(p, np.float64)
    p = p.reshape((-1,) + p.shape[-2:])
    p[:, 0] = 0.0                                                       # row 0 is not read: it counts as zeros
    return p


def solve(lists, mode, x, y, gamma, theta, max_sweeps=1000000):
    """x, y: [P, nS, 5] (or [nS, 5]; the side a mode does not use may be None).  Every policy stops at its own first k with
    max|V_k - V_{k-1}| < theta and keeps that sweep's results.  Returns (br, V, Qr, iterations) with the leading axis P;
    br and Qr are None for EVAL_PAIR; iterations == max_sweeps where a policy did not get there."""
    x = None if x is None else _policies(x)
    y = None if y is None else _policies(y)
    P, nS = (x if x is not None else y).shape[:2]
    V = np.zeros((P, nS)); Qr = np.zeros((P, nS, 5)); br = np.zeros((P, nS), np.int64)
    it = np.full(P, int(max_sweeps), np.int64)
    live = np.arange(P)
    for k in range(1, int(max_sweeps) + 1):
        v, q, b = sweep(lists, mode, None if x is None else x[live], None if y is None else y[live], V[live], gamma)
        d = np.abs(v - V[live]).max(1)
        V[live] = v
        if q is not None:
            Qr[live] = q; br[live] = b
        it[live[d < theta]] = k
        live = live[~(d < theta)]
        if live.size == 0:
            break
    if mode == EVAL_PAIR:
        return None, V, None, it
    return br, V, Qr, it


def best_response(lists, policy, player, gamma, theta, max_sweeps=1000000):
    if player == 0:
        return solve(lists, RESPOND_B, policy, None, gamma, theta, max_sweeps)
    return solve(lists, RESPOND_A, None, policy, gamma, theta, max_sweeps)


def evaluate(lists, pi_a, pi_b, gamma, theta, max_sweeps=1000000):
    _, V, _, it = solve(lists, EVAL_PAIR, pi_a, pi_b, gamma, theta, max_sweeps)
    return V, it


def exploitability(lists, pi_a, pi_b, gamma, theta):
    br_b, v_a, _, k_a = best_response(lists, pi_a, 0, gamma, theta)
    br_a, v_b, _, k_b = best_response(lists, pi_b, 1, gamma, theta)
    return {"v_a": v_a, "v_b": v_b, "gap": v_b - v_a, "br_a": br_a, "br_b": br_b, "iterations": (k_a, k_b)}


def onehot(actions):
    return np.eye(5)[np.asarray(actions, np.int64)]
