"""Minimax (Shapley) value iteration of the two-player game on the device: the stage-game solver against its host build,
the sweep's Q against the host sum over the two-player facade's P[s][(a, b)], value iteration against iterated backups,
and the properties an exact equilibrium solve must have with no LP library and no reference oracle — the eps certificate
of every stage game, the contraction bound, the game's mirror antisymmetry, known values next to the goal, and the
exploitability of the returned strategies.  Then the strategies go into the config-5 rollout, against the CPU oracle."""
import os
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch, SoccerSimultaneousEnv, VectorSoccerEnv
from gym_soccer_littman94_amd import planners as pl
from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_matrix_game_host import assert_certificate, build_games_host, game_set, solve_host  # noqa: E402

pytestmark = pytest.mark.gpu

GAMMA, THETA = 0.9, 1e-10
EAST, WEST = 3, 4
PITCHES = [(5, 4, 0.0), (5, 4, 0.2), (7, 5, 0.3)]


def facade_lists(env):
    """The two-player facade's P[s][(a, b)] as padded arrays [nS, 25, K] in list order (pad: prob 0, reward 0, done)."""
    P = env.P
    nS = env.nS
    K = max(len(P[s][(a, b)]) for s in range(nS) for a in range(5) for b in range(5))
    p = np.zeros((nS, 25, K)); ns = np.zeros((nS, 25, K), np.int64); r = np.zeros((nS, 25, K)); d = np.ones((nS, 25, K), bool)
    for s in range(nS):
        for a in range(5):
            for b in range(5):
                for k, (pr, nxt, rr, dd) in enumerate(P[s][(a, b)]):
                    p[s, a * 5 + b, k] = pr; ns[s, a * 5 + b, k] = nxt; r[s, a * 5 + b, k] = rr; d[s, a * 5 + b, k] = dd
    return p, ns, r, d


def host_q(lists, V, gamma):
    """q = q + prob * (reward + (gamma * V[next]) * (0 if done else 1)), entry by entry in list order (padding adds +-0)."""
    p, ns, r, d = lists
    q = np.zeros(p.shape[:2])
    notdone = np.where(d, 0.0, 1.0)
    for k in range(p.shape[2]):
        q = q + p[:, :, k] * (r[:, :, k] + (gamma * V[ns[:, :, k]]) * notdone[:, :, k])
    return q.reshape(-1, 5, 5)


def sigma_index(env):
    """observation index -> index of the mirrored state (players swapped, columns reflected; EAST <-> WEST)."""
    W = env.width
    rev = {v: k for k, v in env.state_space.items()}
    sig = np.zeros(env.nS, np.int64)
    for s in range(1, env.nS):
        ra, ca, rb, cb, p = rev[s]
        t = (rb, W - 1 - cb, ra, W - 1 - ca, 1 - p)
        assert t in env.state_space, "mirror image of a live state is not a live state"
        sig[s] = env.state_space[t]
    return sig


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_games_host(tmp_path_factory.mktemp("games_gpu"))


_cache = {}


def facade(w, h, slip):
    key = (w, h, slip)
    if key not in _cache:
        env = SoccerSimultaneousEnv(width=w, height=h, slip_prob=slip)
        _cache[key] = (env, facade_lists(env))
    return _cache[key]


def test_solve_matrix_games_bit_identical_to_the_host_build(host):
    A = game_set(np.random.default_rng(1994))
    b = SoccerBatch(1, 5, 4, 0.0)
    v, x, y = b.solve_matrix_games(A)
    hv, hx, hy, sad = solve_host(host, A)
    assert_certificate(A, v, x, y)
    assert set(np.unique(sad).tolist()) == {0, 1, 2}
    np.testing.assert_array_equal(v.view(np.int64), hv.view(np.int64))
    np.testing.assert_array_equal(x.view(np.int64), hx.view(np.int64))
    np.testing.assert_array_equal(y.view(np.int64), hy.view(np.int64))
    b.close()


@pytest.mark.parametrize("w,h,slip", PITCHES)
def test_backup_q_is_the_host_sum_and_every_state_is_certified(w, h, slip):
    env, lists = facade(w, h, slip)
    b = SoccerBatch(1, w, h, slip)
    V = np.random.default_rng(5).uniform(-1, 1, b.nS)
    pa, pb, Vo, Q, _ = b.minimax_backup(V, GAMMA)
    np.testing.assert_array_equal(Q.view(np.int64), host_q(lists, V, GAMMA).view(np.int64))
    assert_certificate(Q, Vo, pa, pb)
    assert (Q[0] == 0).all() and Vo[0] == 0.0 and pa[0, 0] == 1.0 and pb[0, 0] == 1.0
    b.close()


@pytest.mark.parametrize("w,h,slip", PITCHES + [(7, 5, 0.0), (11, 7, 0.2)])
def test_value_iteration_is_iterated_backups(w, h, slip):
    b = SoccerBatch(1, w, h, slip)
    pa, pb, V, Q, k = b.minimax_value_iteration(THETA, GAMMA)
    # the same sweeps from Python, one backup per call
    Vp, it = np.zeros(b.nS), 0
    while True:
        ra, rb, Vn, Qn, _ = b.minimax_backup(Vp, GAMMA)
        assert_certificate(Qn, Vn, ra, rb)                  # every stage game of every sweep
        it += 1
        done = np.abs(Vn - Vp).max() < THETA
        Vp = Vn
        if done:
            break
    assert it == k
    for x, y in ((V, Vp), (Q, Qn), (pa, ra), (pb, rb)):
        np.testing.assert_array_equal(x.view(np.int64), y.view(np.int64))
    assert_certificate(Q, V, pa, pb)
    # a contraction: one more backup moves V by at most gamma * theta + 2 eps
    V2 = b.minimax_backup(V, GAMMA)[2]
    assert np.abs(V2 - V).max() <= GAMMA * THETA + 2e-10
    # same bits again; max_sweeps = k converges, a smaller one (not a multiple of the batch of 16) raises
    again = b.minimax_value_iteration(THETA, GAMMA, max_sweeps=k)
    for x, y in zip((pa, pb, V, Q), again[:4]):
        np.testing.assert_array_equal(x.view(np.int64), y.view(np.int64))
    assert again[4] == k
    m = k - 1 if (k - 1) % 16 else k - 2
    with pytest.raises(RuntimeError):
        b.minimax_value_iteration(THETA, GAMMA, max_sweeps=m)
    b.close()


def check_mirror(env, V):
    sig = sigma_index(env)
    live = np.arange(1, env.nS)
    gap = np.abs(V[sig[live]] + V[live]).max()
    assert gap <= 2 * 1e-10 / (1 - GAMMA), gap
    return gap


@pytest.mark.parametrize("w,h,slip", PITCHES)
def test_mirror_antisymmetry(w, h, slip):
    env, _ = facade(w, h, slip)
    pa, pb, V, Q, k = pl.minimax_value_iteration(env, THETA, GAMMA)
    check_mirror(env, V)
    assert np.abs(V).max() > 0.01


def test_known_values_next_to_the_goal_at_slip_0():
    env, _ = facade(5, 4, 0.0)
    pa, pb, V, Q, k = pl.minimax_value_iteration(env, THETA, GAMMA)
    sig = sigma_index(env)
    W = env.width
    scoring = [s for t, s in env.state_space.items() if s != 0 and t[4] == 0 and t[0] in env.goal_rows and t[1] == W - 2]
    assert len(scoring) == 38
    for s in scoring:
        assert (Q[s, EAST] == 1.0).all() and V[s] == 1.0
        np.testing.assert_array_equal(pa[s], np.eye(5)[EAST])
        assert V[sig[s]] == -1.0


def test_exploitability_without_an_lp_library():
    env, lists = facade(5, 4, 0.2)
    pa, pb, V, Q, k = pl.minimax_value_iteration(env, THETA, GAMMA)
    # best responses to the returned strategies, by value iteration over the same lists in numpy
    br_b = np.zeros(env.nS); br_a = np.zeros(env.nS)
    for _ in range(2000):
        qb = host_q(lists, br_b, GAMMA); qa = host_q(lists, br_a, GAMMA)
        nb = np.einsum("sa,sab->sb", pa, qb).min(1)            # B minimises against pi_a
        na = np.einsum("sab,sb->sa", qa, pb).max(1)            # A maximises against pi_b
        delta = max(np.abs(nb - br_b).max(), np.abs(na - br_a).max())
        br_b, br_a = nb, na
        if delta < 1e-13:
            break
    assert delta < 1e-13
    assert (br_b >= V - 1e-6).all() and (br_a <= V + 1e-6).all()


def test_largest_reference_pitch():
    env = SoccerSimultaneousEnv(width=11, height=7, slip_prob=0.2)
    pa, pb, V, Q, k = pl.minimax_value_iteration(env, THETA, GAMMA)
    assert 0 < k < 1000
    assert_certificate(Q, V, pa, pb)
    b = env._batch
    V2 = b.minimax_backup(V, GAMMA)[2]
    assert np.abs(V2 - V).max() <= GAMMA * THETA + 2e-10
    again = b.minimax_value_iteration(THETA, GAMMA)
    for x, y in zip((pa, pb, V, Q), again[:4]):
        np.testing.assert_array_equal(x.view(np.int64), y.view(np.int64))
    check_mirror(env, V)


def test_validation_capture_and_no_ticks():
    # a single-agent env is refused (AssertionError), on the planner and on the handle
    one = SoccerSimultaneousEnv(width=5, height=4, player_b_policy=[0] * 761)
    with pytest.raises(AssertionError):
        pl.minimax_value_iteration(one, THETA, GAMMA)
    with pytest.raises(AssertionError):
        one._batch.minimax_value_iteration(THETA, GAMMA)
    with pytest.raises(AssertionError):
        one._batch.minimax_backup(np.zeros(761), GAMMA)
    b = SoccerBatch(64, 5, 4, 0.0, seed=1, autoreset=True)
    with pytest.raises(AssertionError):
        b.minimax_value_iteration(THETA, 1.5)
    with pytest.raises(AssertionError):
        b.minimax_value_iteration(THETA, GAMMA, max_sweeps=0)
    # during a graph capture: refused, and the capture still completes
    b.reset()
    n = 64
    A = b.alloc(n, np.int8).fill(0); B = b.alloc(n, np.int8).fill(1)
    obs = b.alloc(n, np.uint16); rew = b.alloc(n, np.int8); term = b.alloc(n, np.uint8); trunc = b.alloc(n, np.uint8)
    b.graph_begin()
    b.step_plain(A, B, obs, rew, term, trunc)
    with pytest.raises(RuntimeError):
        b.minimax_value_iteration(THETA, GAMMA)
    with pytest.raises(RuntimeError):
        b.minimax_backup(np.zeros(761), GAMMA)
    with pytest.raises(RuntimeError):
        b.solve_matrix_games(np.zeros((1, 5, 5)))
    b.graph_destroy(b.graph_end())
    b.close()
    # a solve consumes no tick and leaves the lanes alone: the same rollout with and without one
    outs = []
    for solve in (False, True):
        env = VectorSoccerEnv(4096, slip_prob=0.2, seed=3)
        env.reset()
        if solve:
            tick = env.batch.tick
            pl.minimax_value_iteration(env, THETA, GAMMA)
            env.batch.minimax_backup(np.zeros(env.nS), GAMMA)
            env.batch.solve_matrix_games(np.zeros((3, 5, 5)))
            assert env.batch.tick == tick
        O, R, TE, TR, _ = env.rollout(50, sample_actions=True)
        outs.append((O["player_a"].copy(), R["player_a"].copy(), TE["player_a"].copy(), TR["player_a"].copy()))
        env.close()
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x, y)


def test_config5_rollout_with_minimax_policies_matches_the_oracle():
    """65 536 lanes x 100 steps: minimax pi_a (5x4, slip 0) against uniform B, sampled in the kernel; every step against
    the CPU oracle's replay; A's +1 episodes outnumber its -1 episodes."""
    n, T = 65536, 100
    env, _ = facade(5, 4, 0.0)
    pa, pb, V, Q, k = pl.minimax_value_iteration(env, THETA, GAMMA)
    ta = SoccerBatch.mixed_policy_thresholds(pa)
    np.testing.assert_array_equal(SoccerBatch.mixed_policy_thresholds(pb).shape, (env.nS, 4))
    venv = VectorSoccerEnv(n, 5, 4, 0.0, seed=1994)
    o = Oracle(5, 4, 0.0, n=n, seed=1994, autoreset=True)
    obs0, _ = venv.reset()
    cur = o.reset()
    np.testing.assert_array_equal(obs0["player_a"], cur)
    O, R, TE, TR, _ = venv.rollout(T, sample_actions=True, mixed_policies={"player_a": pa})
    plus = minus = 0
    for t in range(T):
        a, bb = o.sample_actions_mixed(cur, ta, None)
        c = o.step(a, bb)
        np.testing.assert_array_equal(O["player_a"][t], c["obs"])
        np.testing.assert_array_equal(R["player_a"][t], c["reward"].astype(np.float32))
        np.testing.assert_array_equal(TE["player_a"][t], c["terminated"].astype(bool))
        np.testing.assert_array_equal(TR["player_a"][t], c["truncated"].astype(bool))
        plus += int((c["reward"] == 1).sum()); minus += int((c["reward"] == -1).sum())
        cur = c["obs"]
    np.testing.assert_array_equal(venv.episode_histogram(), o.hist)
    print("minimax pi_a vs uniform B, 5x4 slip 0, %d lanes x %d steps: +1 %d  -1 %d  (ratio %.2f)" % (n, T, plus, minus, plus / max(minus, 1)))
    assert plus > minus
    venv.close()
