"""Planners on the device — the reference's `gym_soccer.utils.planners` (gym_soccer/utils/planners.py:4-87)
with the same names, arguments and return values, each running as ONE HIP kernel over transition lists
enumerated on the device (libsoccer_hip.so, include/soccer_hip.h "planners").

Like the reference's they need a single-agent env (one side with a fixed policy); `minimax_value_iteration`, which the
reference lacks, needs the two-player env instead.  The list-based planners
(`value_iteration`, `policy_evaluation`, `policy_improvement`, `policy_iteration`) are bit-identical to the
reference's float64 loops; the dense ones (`policy_eval`, `modified_policy_iteration`) follow its Pmat/Rmat
algebra and agree to rounding (numpy's BLAS dot sums in another order).  `env` is a
`SoccerSimultaneousEnv`, a `VectorSoccerEnv` or a `SoccerBatch` of this package.
"""
import numpy as np


def _batch(env):
    from .core import SoccerBatch
    if isinstance(env, SoccerBatch):
        return env
    b = getattr(env, "_batch", None)
    if b is None:
        raise TypeError("planners expect a gym_soccer_littman94_amd environment")
    assert not env.multiagent, "planners need a single-agent environment (one player with a fixed policy)"
    return b


def value_iteration(env, theta, discount_factor):                        # planners.py:4-18
    return _batch(env).value_iteration(theta, discount_factor)


def policy_evaluation(pi, env, theta, discount_factor):                  # planners.py:20-31
    return _batch(env).policy_evaluation(pi, theta, discount_factor)[0]


def policy_improvement(V, env, discount_factor):                         # planners.py:33-41
    return _batch(env).policy_improvement(V, discount_factor)


def policy_iteration(env, theta, discount_factor, initial_policy=None):  # planners.py:43-53
    b = _batch(env)
    if initial_policy is None:                 # the reference's draw, from numpy's global generator (:45)
        initial_policy = np.random.choice((0, 1, 2, 3, 4), b.nS)
    return b.policy_iteration(initial_policy, theta, discount_factor)


def policy_eval(env, policy, theta, discount_factor, k=10000000, init=None):   # planners.py:55-70
    v, cc = _batch(env).policy_eval_dense(policy, theta, discount_factor, k=k, init=init)
    if init is not None:
        init[:] = v                            # the reference updates `init` in place (v[:] = value_fc) and returns it
        v = init
    return v, cc


def modified_policy_iteration(env, k, theta, discount_factor):           # planners.py:73-87
    return _batch(env).modified_policy_iteration(k, theta, discount_factor)


def _two_player_batch(env, what):
    from .core import SoccerBatch
    if isinstance(env, SoccerBatch):
        return env
    b = getattr(env, "_batch", None)
    if b is None:
        raise TypeError("planners expect a gym_soccer_littman94_amd environment")
    assert env.multiagent, "%s needs a two-player environment (no player with a fixed policy)" % what
    return b


def _train(env, what, factory, n_steps, keys, members=(), **hyper):
    """What the training drivers share: the SoccerBatch factory's learner with `hyper` (decay None: alpha falls to 1 % over
    the run) runs n_steps from the lanes' current states, lanes that were never reset being reset first, and is closed;
    returns read(*members)'s entries `keys`."""
    b = _two_player_batch(env, what)
    n_steps = int(n_steps)
    assert n_steps >= 0, "n_steps must be >= 0"
    if hyper["decay"] is None:
        hyper["decay"] = 0.01 ** (1.0 / max(n_steps, 1))
    learner = getattr(b, factory)(**hyper)
    try:
        if b.get_state()["needs_reset"].any():
            (env if hasattr(env, "_batch") else b).reset()
        learner.run(n_steps)
        r = learner.read(*members)
    finally:
        learner.close()
    return tuple(r[k] for k in keys)


def minimax_q_learning(env, n_steps, discount_factor, alpha=1.0, decay=None, explor=0.2, q_init=1.0, opponent="uniform"):
    """Minimax-Q (Littman 1994) on the device: n_steps learner steps with every lane of `env` acting, from the lanes'
    current states (lanes that were never reset are reset first).  decay None: alpha falls to 1 % over the run.
    Returns (pi_a[nS, 5], pi_b[nS, 5], V, Q[nS, 5, 5], visits[nS, 25]) — minimax_value_iteration's order with the visit
    counts in place of the iteration count, ready for VectorSoccerEnv.rollout(sample_actions=True, mixed_policies={...})."""
    return _train(env, "minimax_q_learning", "minimax_q", n_steps, ("pi_a", "pi_b", "V", "Q", "visits"),
                  discount_factor=discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init, opponent=opponent)


def q_learning(env, n_steps, discount_factor, alpha=1.0, decay=None, explor=0.2, q_init=1.0, act_a="greedy", act_b="greedy"):
    """Independent Q-learning for both players on the device (Littman 1994's baseline and challenger): n_steps learner
    steps with every lane of `env` acting, from the lanes' current states (lanes that were never reset are reset first).
    act_a / act_b: 'greedy', 'uniform' or a fixed [nS, 5] mixed policy; decay None: alpha falls to 1 % over the run.
    Returns (pi_a[nS, 5], pi_b[nS, 5], V_a, V_b, Q_a[nS, 5], Q_b[nS, 5], visits[nS, 25]); the one-hot greedy policies are
    ready for VectorSoccerEnv.rollout(sample_actions=True, mixed_policies={...}) and for exploitability; Q_b and V_b are in
    player B's own reward."""
    return _train(env, "q_learning", "q_learning", n_steps, ("pi_a", "pi_b", "V_a", "V_b", "Q_a", "Q_b", "visits"),
                  discount_factor=discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init, act_a=act_a, act_b=act_b)


def q_population(env, n_steps, discount_factor, alpha=1.0, decay=None, explor=0.2, q_init=1.0, act_a="greedy", act_b="greedy",
                 first=0, count=None, league_policies=None, league_weights=None):
    """A population of independent Q-learners on the device, a learner per lane of `env`, each with its own tables and its
    own stream of experience: n_steps steps of every member from the lanes' current states (lanes that were never reset
    are reset first).  discount_factor, alpha, decay and explor are scalars or arrays of one value per lane; decay None:
    alpha falls to 1 % over the run.  act_a or act_b may be "league" with league_policies [K, nS, 5] and league_weights [K]
    (SoccerBatch.q_population).  Returns, for members first .. first + count - 1 (count None: to the end),
    (pi_a[count, nS, 5], pi_b, V_a[count, nS], V_b, Q_a[count, nS, 5], Q_b, alpha[count]); Q_b and V_b are in player B's
    own reward."""
    return _train(env, "q_population", "q_population", n_steps, ("pi_a", "pi_b", "V_a", "V_b", "Q_a", "Q_b", "alpha"), (first, count),
                  discount_factor=discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init, act_a=act_a, act_b=act_b,
                  league_policies=league_policies, league_weights=league_weights)


def om_population(env, n_steps, discount_factor, alpha=1.0, decay=None, explor=0.2, q_init=1.0, act_a="greedy", act_b="greedy",
                  first=0, count=None):
    """A population of opponent-modelling Q-learners on the device, a learner per lane of `env`, each with its own
    joint-action tables, its own counts of the other player's actions and its own stream of experience: n_steps steps of
    every member from the lanes' current states (lanes that were never reset are reset first).  discount_factor, alpha,
    decay and explor are scalars or arrays of one value per lane; decay None: alpha falls to 1 % over the run.  Returns, for
    members first .. first + count - 1 (count None: to the end), (pi_a[count, nS, 5], pi_b, V_a[count, nS], V_b,
    Q_a[count, nS, 5, 5], Q_b, alpha[count]): the greedy answers to the modelled opponent and their values; Q_b and V_b are
    in player B's own reward."""
    return _train(env, "om_population", "om_population", n_steps, ("pi_a", "pi_b", "V_a", "V_b", "Q_a", "Q_b", "alpha"), (first, count),
                  discount_factor=discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init, act_a=act_a, act_b=act_b)


def wolf_phc(env, n_steps, discount_factor, alpha=1.0, decay=None, explor=0.2, q_init=1.0, delta_win=0.01, delta_lose=0.04,
             delta_decay=1.0, act_a="learn", act_b="learn"):
    """PHC / WoLF-PHC (Bowling & Veloso 2002) for both players on the device: n_steps learner steps with every lane of
    `env` acting, from the lanes' current states (lanes that were never reset are reset first).  act_a / act_b: 'learn',
    'uniform' or a fixed [nS, 5] mixed policy; decay None: alpha falls to 1 % over the run; delta_win == delta_lose is
    plain PHC.  Returns (pi_a[nS, 5], pi_b[nS, 5], avg_a, avg_b, Q_a[nS, 5], Q_b[nS, 5], visits[nS, 25]); the policies and
    their averages are ready for VectorSoccerEnv.rollout(sample_actions=True, mixed_policies={...}) and for
    exploitability; Q_b is in player B's own reward."""
    return _train(env, "wolf_phc", "wolf_phc", n_steps, ("pi_a", "pi_b", "avg_a", "avg_b", "Q_a", "Q_b", "visits"),
                  discount_factor=discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init,
                  delta_win=delta_win, delta_lose=delta_lose, delta_decay=delta_decay, act_a=act_a, act_b=act_b)


def wolf_population(env, n_steps, discount_factor, alpha=1.0, decay=None, explor=0.2, q_init=1.0, delta_win=0.01, delta_lose=0.04,
                    delta_decay=1.0, act_a="learn", act_b="learn", first=0, count=None):
    """A population of PHC / WoLF-PHC learners on the device, a learner per lane of `env`, each with its own tables,
    policies and stream of experience: n_steps steps of every member from the lanes' current states (lanes that were never
    reset are reset first).  The hyperparameters are scalars or arrays of one value per lane; decay None: alpha falls to
    1 % over the run; act_a / act_b: 'learn', 'uniform', a fixed [nS, 5] policy or [n, nS, 5], one per member.  Returns, for
    members first .. first + count - 1 (count None: to the end), (pi_a[count, nS, 5], pi_b, avg_a, avg_b, Q_a, Q_b,
    alpha[count]); Q_b is in player B's own reward."""
    return _train(env, "wolf_population", "wolf_population", n_steps, ("pi_a", "pi_b", "avg_a", "avg_b", "Q_a", "Q_b", "alpha"), (first, count),
                  discount_factor=discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init,
                  delta_win=delta_win, delta_lose=delta_lose, delta_decay=delta_decay, act_a=act_a, act_b=act_b)


def regret_population(env, n_steps, discount_factor, alpha=1.0, decay=None, explor=0.2, q_init=1.0, plus=True, linear=False,
                      act_a="learn", act_b="learn", first=0, count=None):
    """A population of regret matchers on the device, a learner per lane of `env`, each with its own tables, regrets, policy
    sums and stream of experience: n_steps steps of every member from the lanes' current states (lanes that were never reset
    are reset first).  discount_factor, alpha, decay and explor are scalars or arrays of one value per lane; decay None: alpha
    falls to 1 % over the run; plus: regret matching+; linear: linear averaging; act_a / act_b: 'learn', 'uniform', a fixed
    [nS, 5] policy or [n, nS, 5], one per member.  Returns, for members first .. first + count - 1 (count None: to the end),
    (avg_a[count, nS, 5], avg_b, pi_a, pi_b, Q_a, Q_b, alpha[count]): the average policies first, they carry the guarantee; Q_b
    is in player B's own reward."""
    return _train(env, "regret_population", "regret_population", n_steps, ("avg_a", "avg_b", "pi_a", "pi_b", "Q_a", "Q_b", "alpha"), (first, count),
                  discount_factor=discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init, plus=plus, linear=linear,
                  act_a=act_a, act_b=act_b)


def regret_matching(env, n_steps, discount_factor, alpha=1.0, decay=None, explor=0.2, q_init=1.0, plus=True, linear=False,
                    act_a="learn", act_b="learn"):
    """Regret matching for both players on the device with one table that every lane of `env` feeds (the shared form of
    regret_population): n_steps learner steps from the lanes' current states (lanes that were never reset are reset first).
    decay None: alpha falls to 1 % over the run; plus: regret matching+; linear: linear averaging; act_a / act_b: 'learn',
    'uniform' or a fixed [nS, 5] mixed policy.  Returns (avg_a[nS, 5], avg_b, pi_a, pi_b, Q_a[nS, 5], Q_b, visits[nS, 25]): the
    average policies first, they carry the guarantee; Q_b is in player B's own reward."""
    return _train(env, "regret_matching", "regret_matching", n_steps, ("avg_a", "avg_b", "pi_a", "pi_b", "Q_a", "Q_b", "visits"),
                  discount_factor=discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init, plus=plus, linear=linear,
                  act_a=act_a, act_b=act_b)


def minimax_q_population(env, n_steps, discount_factor, alpha=1.0, decay=None, explor=0.2, q_init=1.0, opponent="uniform", first=0,
                         count=None):
    """A population of minimax-Q learners on the device, a learner per lane of `env`, each with its own table, strategies
    and stream of experience: n_steps steps of every member from the lanes' current states (lanes that were never reset
    are reset first).  discount_factor, alpha, decay and explor are scalars or arrays of one value per lane; decay None:
    alpha falls to 1 % over the run; opponent: 'uniform', 'self', a fixed [nS, 5] policy or [n, nS, 5], one per member.
    Returns, for members first .. first + count - 1 (count None: to the end), (pi_a[count, nS, 5], pi_b, V[count, nS],
    Q[count, nS, 5, 5], alpha[count])."""
    return _train(env, "minimax_q_population", "minimax_q_population", n_steps, ("pi_a", "pi_b", "V", "Q", "alpha"), (first, count),
                  discount_factor=discount_factor, alpha=alpha, decay=decay, explor=explor, q_init=q_init, opponent=opponent)


def minimax_value_iteration(env, theta, discount_factor, max_sweeps=1000000):
    """Minimax (Shapley) value iteration of the two-player game on the device, Littman (1994)'s equilibrium values.
    Returns (pi_a[nS, 5], pi_b[nS, 5], V, Q[nS, 5, 5], iterations): player A's maximin and player B's minimax stage-game
    strategies, ready for VectorSoccerEnv.rollout(sample_actions=True, mixed_policies={...}).  RuntimeError if max_sweeps is
    reached: the handle's exception passes through, its .results holding the tuple of sweep max_sweeps."""
    return _two_player_batch(env, "minimax_value_iteration").minimax_value_iteration(theta, discount_factor, max_sweeps=max_sweeps)


def best_response(env, policy, player, theta, discount_factor, max_sweeps=1000000):
    """The best response to a mixed policy of `player` (0: player A's policy, B answers; 1: player B's, A answers) in the
    two-player game, on the device (include/soccer_hip.h, "best responses").  policy is [nS, 5], or [P, nS, 5] for a batch
    solved in one sequence of launches.  Returns (br, V, Qr, iterations) like value_iteration; V is player A's value,
    i.e. the policy's worst case."""
    return _two_player_batch(env, "best_response").best_response(policy, player, theta, discount_factor, max_sweeps=max_sweeps)


def exploitability(env, pi_a, pi_b, theta, discount_factor, max_sweeps=1000000):
    """How badly the best possible opponent beats each of two mixed policies: one best-response solve per side.  Either
    policy is [nS, 5] or a batch [P, nS, 5].  Returns a dict, everything from player A's side:
      v_a   worst case of pi_a (B answers it): a lower bound on the game's value
      v_b   worst case of pi_b (A answers it): an upper bound
      gap   v_b - v_a per state, >= 0 up to theta, and 0 exactly at an equilibrium pair
      br_a  player A's best-response actions to pi_b,  br_b  player B's to pi_a
      iterations  (sweeps of the solve behind v_a, sweeps of the solve behind v_b)"""
    b = _two_player_batch(env, "exploitability")
    br_b, v_a, _, k_a = b.best_response(pi_a, 0, theta, discount_factor, max_sweeps=max_sweeps)
    br_a, v_b, _, k_b = b.best_response(pi_b, 1, theta, discount_factor, max_sweeps=max_sweeps)
    return {"v_a": v_a, "v_b": v_b, "gap": v_b - v_a, "br_a": br_a, "br_b": br_b, "iterations": (k_a, k_b)}


def cross_play(env, pi_a, pi_b, theta, discount_factor, max_sweeps=1000000):
    """The cross-play (tournament) matrix of two sets of mixed policies, on the device (include/soccer_hip.h, "cross-play"):
    pi_a is [n_a, nS, 5], pi_b [n_b, nS, 5].  Returns a dict, everything player A's value at kick-off:
      payoff      [n_a, n_b], pi_a[i] against pi_b[j]
      iterations  [n_a, n_b], the sweeps of each pair's solve
      row_min     [n_a] each A policy against its worst opponent in the set,  col_max  [n_b] likewise each B policy
      bounds      (row_min.max(), col_max.min()): the pure maximin and minimax, which bracket the meta-game's value"""
    payoff, it = _two_player_batch(env, "cross_play").cross_play(pi_a, pi_b, theta, discount_factor, max_sweeps=max_sweeps)
    row_min, col_max = payoff.min(1), payoff.max(0)
    return {"payoff": payoff, "iterations": it, "row_min": row_min, "col_max": col_max,
            "bounds": (float(row_min.max()), float(col_max.min()))}


def match_outcomes(env, pi_a, pi_b, theta, continue_prob, max_sweeps=1000000):
    """Littman's columns for two sets of mixed policies, exactly, on the device (include/soccer_hip.h, "match outcomes"): after
    every step the game goes on with probability continue_prob and is a draw otherwise.  pi_a is [n_a, nS, 5], pi_b
    [n_b, nS, 5].  Returns a dict of [n_a, n_b] arrays at kick-off: win_a, win_b, draw = 1 - win_a - win_b, length (steps per
    game), games_per_step = 1 / length and iterations."""
    return _two_player_batch(env, "match_outcomes").match_outcomes(pi_a, pi_b, theta, continue_prob, max_sweeps=max_sweeps)


def occupancy(env, pi_a, pi_b, theta, continue_prob, features=None, values=False, max_sweeps=1000000):
    """Where the game is played when two sets of mixed policies meet, exactly, on the device (include/soccer_hip.h, "state
    occupancy"): the expected number of visits to every state from kick-off when after every step the game goes on with
    probability continue_prob.  pi_a is [n_a, nS, 5], pi_b [n_b, nS, 5], features [n_f, nS] (pitch_features' vectors, for
    instance).  Returns a dict: length [n_a, n_b], expect [n_a, n_b, n_f] = sum_s occupancy * features, iterations, and with
    values=True occupancy [n_a, n_b, nS] and visit_share = occupancy / length."""
    return _two_player_batch(env, "occupancy").occupancy(pi_a, pi_b, theta, continue_prob, features=features, values=values,
                                                         max_sweeps=max_sweeps)


def policy_gradient(env, pi_a, pi_b, theta, discount_factor, w_a=None, w_b=None, normalize=False, values=False, max_sweeps=1000000):
    """The exact policy gradients of two sets of mixed policies, on the device (include/soccer_hip.h, "exact policy
    gradients"): grad_a[i] is the gradient of sum_j w_b[j] * payoff(pi_a[i], pi_b[j]) in pi_a[i] under the direct
    parametrisation, occupancy times action value, and grad_b[j] that of sum_i w_a[i] * payoff(pi_a[i], pi_b[j]) in pi_b[j]
    (player A's payoff: B descends it).  Returns SoccerBatch.policy_gradient's dict."""
    return _two_player_batch(env, "policy_gradient").policy_gradient(pi_a, pi_b, theta, discount_factor, w_a=w_a, w_b=w_b,
                                                                     normalize=normalize, values=values, max_sweeps=max_sweeps)


def gradient_play(env, n_steps, discount_factor, n_a=1, n_b=1, eta_a=1.0, eta_b=1.0, optimism=0.0, normalize=True, theta=1e-10,
                  max_sweeps=1000000, pi_a=None, pi_b=None, w_a=None, w_b=None):
    """n_steps of gradient play on the device from pi_a / pi_b (None: uniform): every policy follows the exact gradient of its
    payoff against the other side's weighted mixture, projected onto the simplex row by row.  Returns read()'s dict (pi_a, pi_b,
    prev_a, prev_b, w_a, w_b, payoff, steps) plus trace [n_steps, n_a, n_b], each step's payoff matrix before its update."""
    g = _two_player_batch(env, "gradient_play").gradient_play(n_a=n_a, n_b=n_b, discount_factor=discount_factor, eta_a=eta_a, eta_b=eta_b,
                                                              optimism=optimism, normalize=normalize, theta=theta,
                                                              max_sweeps=max_sweeps, pi_a=pi_a, pi_b=pi_b)
    try:
        if w_a is not None or w_b is not None:
            g.weights(w_a, w_b)
        trace = g.run(n_steps, trace=True)
        out = g.read()
    finally:
        g.close()
    out["trace"] = trace
    return out


def pitch_features(env):
    """Per-state vectors [nS] decoded from the handle's tables, to weigh an occupancy with (occupancy's features, or a dot
    product with its values): possession_a / possession_b (1.0 where that side has the ball), row_a, col_a, row_b, col_b (the
    players' squares, in the coordinates of the handle's state) and ball_row / ball_col (the square of the side that has the
    ball).  State 0, the end of the game, is 0.0 in all of them."""
    b = getattr(env, "_batch", env)                                     # (any environment of the package, or a SoccerBatch)
    lut = b.tables()[0].astype(np.int64)
    W, H = b.internal_width, b.height
    f = np.flatnonzero((lut != 0) & (lut != 0xFFFF))
    s = lut[f]
    p = f & 1; r = f >> 1
    cb = r % W; r //= W; rb = r % H; r //= H; ca = r % W; ra = r // W
    out = {}
    for name, v in (("possession_a", p == 0), ("possession_b", p == 1), ("row_a", ra), ("col_a", ca), ("row_b", rb), ("col_b", cb),
                    ("ball_row", np.where(p == 0, ra, rb)), ("ball_col", np.where(p == 0, ca, cb))):
        out[name] = np.zeros(b.nS)
        out[name][s] = v
    return out


def collapse_occupancies(policies, weights, D):
    """The one Markov policy that plays like a kick-off mixture: sigma[s] = sum_k w_k D_k[s] policies[k][s] / sum_k w_k D_k[s]
    for policies [K, nS, 5], weights [K] and the members' occupancies D [K, nS] against one opponent; uniform where the
    denominator is 0 (the mixture never gets there).  Returns (sigma[nS, 5], the mixture's occupancy sum_k w_k D_k [nS]).
    Sums run over ascending k in float64."""
    policies = np.asarray(policies, np.float64); weights = np.asarray(weights, np.float64); D = np.asarray(D, np.float64)
    K, nS = policies.shape[:2]
    assert policies.shape == (K, nS, 5) and weights.shape == (K,) and D.shape == (K, nS)
    den = np.zeros(nS); num = np.zeros((nS, 5))
    for k in range(K):
        wd = weights[k] * D[k]
        den = den + wd
        num = num + wd[:, None] * policies[k]
    with np.errstate(divide="ignore", invalid="ignore"):
        sigma = np.where(den[:, None] > 0, num / den[:, None], 0.2)
    return sigma, den


def collapse_mixture(env, policies, weights, player, opponent, theta, continue_prob, max_sweeps=1000000):
    """A league as a single Markov policy, against a given opponent.  Drawing policies[k] with probability weights[k] at
    kick-off and keeping it for the game is not the state-wise average sum_k w_k policies[k]: the members reach a state
    with different probabilities.  Weighted by the members' occupancies D_k against `opponent` ([nS, 5]; occupancy on the
    device) it is a Markov policy: collapse_occupancies' sigma visits every state as often as the mixture does and scores
    what the mixture scores, against this opponent.  player 0: the policies are player A's and the opponent is B's, 1: the
    other way round.  Returns (sigma[nS, 5], occupancy[nS])."""
    assert player in (0, 1), "player must be 0 (the policies are player A's) or 1 (player B's)"
    b = _two_player_batch(env, "collapse_mixture")
    policies = np.asarray(policies, np.float64)
    sides = (policies, opponent) if player == 0 else (opponent, policies)
    D = b.occupancy(sides[0], sides[1], theta, continue_prob, values=True, max_sweeps=max_sweeps)["occupancy"]
    return collapse_occupancies(policies, weights, D.reshape(policies.shape[0], -1))


def meta_game(env, pi_a, pi_b, theta, discount_factor, max_sweeps=1000000, max_pivots=None):
    """cross_play followed by the solve of its meta-game, both on the device (include/soccer_hip.h, "the meta-game"): which
    mixture of player A's policies can a rational mixture of player B's not beat?  Returns cross_play's dict plus
      x [n_a], y [n_b]  the maximin mixture of A's policies and the minimax mixture of B's
      lo, hi, value     what x guarantees, what y concedes at most (lo <= the meta-game's value <= hi), their midpoint
      status            1 saddle point, 0 hi - lo <= 1e-10 * max(1, max|payoff|), 2 finished but wider
      gain              lo - bounds[0]: what mixing buys player A over the best single policy
    max_pivots None: 100 * (n_a + n_b); RuntimeError if the solve stops there."""
    from .core import _meta_of_cross_play
    batch = _two_player_batch(env, "meta_game")
    payoff, it = batch.cross_play(pi_a, pi_b, theta, discount_factor, max_sweeps=max_sweeps)
    return _meta_of_cross_play(batch, payoff, it, max_pivots)


PSRO_MAX_POLICIES = 1024        # what cross_play, solve_meta_game and a league take a side


def _weighted(P, w):
    """sum_j w[j] * P[:, j], sequentially in ascending j in float64"""
    u = np.zeros(P.shape[0])
    for j in range(P.shape[1]):
        u = u + float(w[j]) * P[:, j]
    return u


def psro(env, iterations, n_steps, discount_factor, theta=1e-10, pi_a0=None, pi_b0=None, **q_hyper):
    """Policy-space response oracles (double oracle with learned responses) on the device, built from cross_play, the
    meta-game and league challengers.  `env` is a two-player autoreset env whose n lanes are the challengers.  The policy
    sets start as pi_a0 / pi_b0 ([nS, 5] or [k, nS, 5]; None: the uniform policy).  Per iteration:
      1. the payoff matrix of the sets Pi_A x Pi_B is extended by the new row and the new column alone (every pair has the
         bits it has alone, so the matrix equals a full cross_play(Pi_A, Pi_B) bit for bit)
      2. solve_meta_game gives x, y, lo, hi, status
      3. a fresh population with act_a="greedy" against the league (Pi_B, y) runs n_steps, then a fresh one with
         act_b="greedy" against the league (Pi_A, x); q_hyper (alpha, decay, explor, q_init) goes to both, decay None:
         alpha falls to 1 % over the run
      4. every member's one-hot greedy policy is scored exactly: u_a[i] = sum_j y_j * cross_play(candidate_i, Pi_B[j]),
         summed in ascending j; u_b[i] likewise with x.  A's pick is the first argmax of u_a, B's the first argmin of u_b
      5. A's pick joins Pi_A only if u_a[pick] > hi, B's joins Pi_B only if u_b[pick] < lo; a set stops growing at 1024
    Returns a dict: pi_a, pi_b (the final sets), payoff and iterations (their matrix and its sweep counts), and per
    iteration the lists x, y, lo, hi, status, chosen_a, chosen_b, added_a, added_b, br_a = u_a[chosen_a], br_b, gap =
    br_a - br_b, with u_a, u_b as [iterations, n] arrays.
    gap is a LOWER estimate of the NashConv of the mixture pair (x, y) in the full game: the challengers are learners, not
    exact best responses.  The exact best response to a kick-off mixture is a partially observed problem (the responder
    does not see which policy was drawn) and is out of scope here."""
    b = _two_player_batch(env, "psro")
    iterations, n_steps = int(iterations), int(n_steps)
    assert iterations >= 0 and n_steps >= 0, "iterations and n_steps must be >= 0"
    nS, n = b.nS, b.n
    gamma = float(discount_factor)
    hyper = dict(q_hyper)
    if hyper.get("decay") is None:
        hyper["decay"] = 0.01 ** (1.0 / max(n_steps, 1))
    assert not {"act_a", "act_b", "league_policies", "league_weights"} & set(hyper), "psro sets the players of its challengers itself"

    def seed(pi, name):
        if pi is None:
            return np.full((1, nS, 5), 0.2)
        pi = np.array(pi, np.float64)
        pi = pi[None] if pi.ndim == 2 else pi
        assert pi.ndim == 3 and pi.shape[1:] == (nS, 5) and 1 <= pi.shape[0] <= PSRO_MAX_POLICIES, "%s must be [n_states, 5] or [k, n_states, 5]" % name
        return pi
    Pa, Pb = seed(pi_a0, "pi_a0"), seed(pi_b0, "pi_b0")
    payoff, sweeps = b.cross_play(Pa, Pb, theta, gamma)
    out = {k: [] for k in ("x", "y", "lo", "hi", "status", "chosen_a", "chosen_b", "added_a", "added_b", "br_a", "br_b", "gap")}
    U = {0: [], 1: []}

    def challengers(learner, league, weights):
        """[n, nS, 5]: the greedy policies `learner` (0 = A, 1 = B) has learned against the league after n_steps"""
        acts = {"act_a": "greedy", "act_b": "league"} if learner == 0 else {"act_a": "league", "act_b": "greedy"}
        pop = b.q_population(gamma, league_policies=league, league_weights=weights, **acts, **hyper)
        try:
            if b.get_state()["needs_reset"].any():
                (env if hasattr(env, "_batch") else b).reset()
            pop.run(n_steps)
            cand = np.zeros((n, nS, 5))
            for c0 in range(0, n, 256):
                c = min(256, n - c0)
                cand[c0:c0 + c] = pop.read(c0, c)["pi_b" if learner else "pi_a"]
        finally:
            pop.close()
        return cand

    def score(cand, learner, others, weights):
        u = np.zeros(n)
        for c0 in range(0, n, PSRO_MAX_POLICIES):
            c = cand[c0:c0 + PSRO_MAX_POLICIES]
            P = b.cross_play(c, others, theta, gamma)[0] if learner == 0 else b.cross_play(others, c, theta, gamma)[0].T
            u[c0:c0 + c.shape[0]] = _weighted(P, weights)
        return u

    for _ in range(iterations):
        m = b.solve_meta_game(payoff)
        x, y, lo, hi = m["x"].copy(), m["y"].copy(), float(m["lo"]), float(m["hi"])
        cand_a = challengers(0, Pb, y)
        cand_b = challengers(1, Pa, x)
        u_a, u_b = score(cand_a, 0, Pb, y), score(cand_b, 1, Pa, x)
        ia, ib = int(np.argmax(u_a)), int(np.argmin(u_b))
        add_a = bool(u_a[ia] > hi) and Pa.shape[0] < PSRO_MAX_POLICIES
        add_b = bool(u_b[ib] < lo) and Pb.shape[0] < PSRO_MAX_POLICIES
        for k, v in (("x", x), ("y", y), ("lo", lo), ("hi", hi), ("status", int(m["status"])), ("chosen_a", ia), ("chosen_b", ib),
                     ("added_a", add_a), ("added_b", add_b), ("br_a", float(u_a[ia])), ("br_b", float(u_b[ib])),
                     ("gap", float(u_a[ia]) - float(u_b[ib]))):
            out[k].append(v)
        U[0].append(u_a); U[1].append(u_b)
        # the new column against the old rows, then the new row against every column
        if add_b:
            col, col_it = b.cross_play(Pa, cand_b[ib], theta, gamma)
            Pb = np.concatenate([Pb, cand_b[ib][None]])
            payoff, sweeps = np.concatenate([payoff, col], 1), np.concatenate([sweeps, col_it], 1)
        if add_a:
            row, row_it = b.cross_play(cand_a[ia], Pb, theta, gamma)
            Pa = np.concatenate([Pa, cand_a[ia][None]])
            payoff, sweeps = np.concatenate([payoff, row], 0), np.concatenate([sweeps, row_it], 0)
    out.update({"pi_a": Pa, "pi_b": Pb, "payoff": payoff, "iterations": sweeps,
                "u_a": np.array(U[0]).reshape(iterations, n), "u_b": np.array(U[1]).reshape(iterations, n)})
    return out
