"""The single-agent planners on the device (planner_kernel; include/soccer_hip.h, "planners") on every size at which the launch
takes another path: fewer states than the workgroup's 1024 threads (5x4), several states per thread (7x5, 9x6: the last pitch
under the default 48 KiB of dynamic LDS), the raised LDS limit (8x7 and 7x8: 136 bytes over it; 11x7), the largest pitch
build_plan accepts (14x7) and the first it refuses (13x8).  Bit for bit the numpy restatement over the CPU oracle's lists
(tests/planners_np.py) for all six planners; on 5x4 and 7x5 the dense ones also to rounding against the oracle's dense numpy
versions; results that do not depend on what earlier calls left in the handle's buffers; the outputs at the sweep cap; the
dense lists unchanged by building the rows sparsely (tests/golden/planner_dense_7x5_s0p3.npz, recorded from the build before
that change), and the host memory a first planner call takes."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch
from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planners_np as pn  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
THETA, GAMMA = 1e-8, 0.9
DENSE_RTOL, DENSE_ATOL = 1e-12, 1e-14                          # tests/test_planner.py's bound against numpy's BLAS dot
# width, height, slip, learner
PITCHES = [(5, 4, 1.0, "player_a"), (7, 5, 0.3, "player_b"), (9, 6, 0.1, "player_a"), (8, 7, 0.2, "player_b"),
           (11, 7, 0.2, "player_a"), (14, 7, 0.2, "player_b"), (7, 8, 0.0, "player_a")]
LARGEST, REFUSED = (14, 7), (13, 8)                            # 152 104 and 171 400 bytes of V: either side of build_plan's bound
IDS = ["%dx%d" % p[:2] for p in PITCHES]
MPI = [(1, THETA), (5, 1e-6), (10 ** 7, THETA)]

class Game:
    """one pitch: the oracle's lists and rows, the fixed policy, the inputs of every test and a handle, built once"""

    def __init__(self, w, h, slip, learner):
        self.w, self.h, self.slip, self.learner = w, h, slip, learner
        orc = O.Oracle(w, h, slip)
        self.nS = orc.nS
        rng = np.random.default_rng(w * 100 + h)
        self.opponent = rng.integers(0, 5, self.nS).astype(np.int8)
        self.lists, self.rows = pn.from_oracle(orc, learner, self.opponent)
        self.pi = rng.integers(0, 5, self.nS)                   # a deterministic policy to evaluate
        self.pi0 = rng.integers(0, 5, self.nS)                  # policy iteration's start
        self.V = rng.uniform(-1, 1, self.nS)                    # policy improvement's input
        self.policy = rng.dirichlet(np.ones(5), self.nS)        # dense evaluation's stochastic policy
        self.init = rng.uniform(-1, 1, self.nS)
        self.batch = self.fresh()
        self.ref = {}

    def fresh(self):
        b = SoccerBatch(1, self.w, self.h, self.slip)
        b.set_policy("player_b" if self.learner == "player_a" else "player_a", self.opponent)
        return b

    def want(self, name, call):
        """a result of the restatement, computed once"""
        if name not in self.ref:
            self.ref[name] = call()
        return self.ref[name]


@pytest.fixture(scope="module")
def game():
    """(w, h, slip, learner) -> Game, built once for this module; afterwards the handles are closed and the lists dropped"""
    games = {}

    def get(w, h, slip, learner):
        key = (w, h, slip, learner)
        if key not in games:
            games[key] = Game(w, h, slip, learner)
        return games[key]

    yield get
    for g in games.values():
        g.batch.close()
    games.clear()


def same_bits(got, want, what):
    g = np.ascontiguousarray(got); w = np.ascontiguousarray(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if g.dtype == np.float64:
        g = g.view(np.int64); w = np.ascontiguousarray(w, np.float64).view(np.int64)
    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    assert bad.size == 0, "%s differs in %d entries, first at flat index %d: %r vs %r" % (
        what, bad.size, bad[0], np.asarray(got).reshape(-1)[bad[0]], np.asarray(want).reshape(-1)[bad[0]])


def same_plan(got, want, what):
    """got: (pi, V, Q, counter) of a device call"""
    pi, V, Q, counter = got
    assert counter == want.counter, "%s: counter %d, the restatement's %d" % (what, counter, want.counter)
    same_bits(V, want.V, what + " V"); same_bits(Q, want.Q, what + " Q"); same_bits(pi, want.pi, what + " pi")


def test_the_pitches_sit_where_the_launch_changes(game):
    nS = {(w, h): 2 * w * h * (w * h - 1) + 1 for w, h in [p[:2] for p in PITCHES] + [REFUSED]}
    for (w, h, slip, learner) in PITCHES:
        assert game(w, h, slip, learner).nS == nS[(w, h)]
    assert nS[(5, 4)] < 1024 < nS[(7, 5)]
    assert 8 * nS[(9, 6)] <= 48 * 1024 < 8 * nS[(8, 7)] and nS[(7, 8)] == nS[(8, 7)]
    assert 8 * nS[LARGEST] <= 150 * 1024 < 8 * nS[REFUSED]
    assert {p[3] for p in PITCHES} == {"player_a", "player_b"}


# ---- 1. bit for bit against the restatement, every pitch -------------------------------------------------------------------
@pytest.mark.parametrize("w,h,slip,learner", PITCHES, ids=IDS)
def test_value_iteration(w, h, slip, learner, game):
    g = game(w, h, slip, learner)
    want = g.want("vi", lambda: pn.value_iteration(g.lists, THETA, GAMMA))
    assert not want.capped and want.counter > 20
    same_plan(g.batch.value_iteration(THETA, GAMMA), want, "value iteration")


@pytest.mark.parametrize("w,h,slip,learner", PITCHES, ids=IDS)
def test_policy_evaluation_and_improvement(w, h, slip, learner, game):
    g = game(w, h, slip, learner)
    want = g.want("pe", lambda: pn.policy_evaluation(g.lists, g.pi, THETA, GAMMA))
    V, sweeps = g.batch.policy_evaluation(g.pi, THETA, GAMMA)
    assert sweeps == want.counter and not want.capped
    same_bits(V, want.V, "policy evaluation V")
    want = g.want("imp", lambda: pn.policy_improvement(g.lists, g.V, GAMMA))
    pi, Q = g.batch.policy_improvement(g.V, GAMMA)
    same_bits(Q, want.Q, "policy improvement Q"); same_bits(pi, want.pi, "policy improvement pi")


PI_SWEEPS = 5000                                               # several times what any pitch here needs to converge


@pytest.mark.parametrize("w,h,slip,learner", PITCHES, ids=IDS)
def test_policy_iteration(w, h, slip, learner, game):
    """Policy iteration stops when an improvement changes nothing.  At slip 1.0 the intended move is never made, many actions
    of a state are worth the same up to the rounding of an evaluation stopped at theta, and the first argmax goes on flipping
    between them: the reference's loop does not end there, and neither does the restatement or the kernel.  So every pitch
    runs under the same cap, through the C ABI: where the iteration converges (everywhere but at slip 1.0) the call succeeds,
    where it does not the call ends with SOCCER_E_STATE, and either way the outputs are the restatement's bit for bit."""
    g = game(w, h, slip, learner)
    want = g.want("pi", lambda: pn.policy_iteration(g.lists, g.pi0, THETA, GAMMA, max_sweeps=PI_SWEEPS))
    assert want.capped == (slip == 1.0) and want.counter >= 2
    rc, V, Q, pi, counter = _raw(g.batch, "soccer_policy_iteration", g.pi0, THETA, GAMMA, PI_SWEEPS)
    assert rc == (_e_state() if want.capped else 0), (rc, g.batch.lib.soccer_last_error(g.batch.h))
    same_plan((pi, V, Q, counter), want, "policy iteration")


def test_policy_iteration_converges_with_fewer_states_than_threads(game):
    """5x4 at slip 1.0 above only ever ends at the cap; at slip 0.2 the same pitch converges (7 improvements, several hundred
    sweeps), which makes it the converged policy iteration with idle threads in the workgroup"""
    g = game(5, 4, 0.2, "player_b")
    assert g.nS < 1024
    want = g.want("pi", lambda: pn.policy_iteration(g.lists, g.pi0, THETA, GAMMA, max_sweeps=PI_SWEEPS))
    assert not want.capped and want.counter >= 3 and want.sweeps > 100
    same_plan(g.batch.policy_iteration(g.pi0, THETA, GAMMA), want, "policy iteration")


@pytest.mark.parametrize("w,h,slip,learner", PITCHES, ids=IDS)
def test_policy_eval_dense(w, h, slip, learner, game):
    g = game(w, h, slip, learner)
    want = g.want("de7", lambda: pn.policy_eval_dense(g.rows, g.policy, THETA, GAMMA, k=7, init=g.init))
    assert want.counter == 7 and not want.capped                # stops on k, not on theta
    v, cc = g.batch.policy_eval_dense(g.policy, THETA, GAMMA, k=7, init=g.init.copy())
    assert cc == 7
    same_bits(v, want.V, "dense evaluation, k = 7 from init")
    want = g.want("de0", lambda: pn.policy_eval_dense(g.rows, g.policy, THETA, GAMMA))
    v, cc = g.batch.policy_eval_dense(g.policy, THETA, GAMMA)
    assert cc == want.counter and cc > 7 and not want.capped
    same_bits(v, want.V, "dense evaluation from zeros")


@pytest.mark.parametrize("k,theta", MPI, ids=["k1", "k5", "k1e7"])
@pytest.mark.parametrize("w,h,slip,learner", PITCHES, ids=IDS)
def test_modified_policy_iteration(w, h, slip, learner, k, theta, game):
    g = game(w, h, slip, learner)
    want = g.want(("mpi", k), lambda: pn.modified_policy_iteration(g.rows, k, theta, GAMMA))
    assert not want.capped and want.counter >= 2
    same_plan(g.batch.modified_policy_iteration(k, theta, GAMMA), want, "modified policy iteration, k = %d" % k)


@pytest.mark.parametrize("w,h,slip,learner", PITCHES[:2], ids=IDS[:2])
def test_dense_planners_against_the_oracle_numpy_versions(w, h, slip, learner, game):
    """numpy's BLAS dot associates differently from the kernel's sequential one: equal to rounding, with the same counters and
    greedy policy.  Only where Pmat[nS, nS, 5] fits in memory."""
    g = game(w, h, slip, learner)
    Pmat, Rmat = pn.densify(g.rows)
    v0, cc0 = O.policy_eval_dense(Pmat, Rmat, g.policy, THETA, GAMMA, k=7, init=g.init.copy())
    v, cc = g.batch.policy_eval_dense(g.policy, THETA, GAMMA, k=7, init=g.init.copy())
    assert cc == cc0
    np.testing.assert_allclose(v, v0, rtol=DENSE_RTOL, atol=DENSE_ATOL)
    pi0, V0, Q0, c0 = O.modified_policy_iteration(Pmat, Rmat, 5, 1e-6, GAMMA)
    pi, V, Q, c = g.batch.modified_policy_iteration(5, 1e-6, GAMMA)
    assert c == c0 and np.array_equal(pi, pi0)
    np.testing.assert_allclose(V, V0, rtol=DENSE_RTOL, atol=DENSE_ATOL)
    np.testing.assert_allclose(Q, Q0, rtol=DENSE_RTOL, atol=DENSE_ATOL)


# ---- 2. the bound -----------------------------------------------------------------------------------------------------------
def test_the_first_pitch_over_the_bound_is_refused_and_the_handle_still_steps():
    w, h = REFUSED
    n = 64
    b = SoccerBatch(n, w, h, 0.2, seed=5, autoreset=True)
    rng = np.random.default_rng(3)
    b.set_policy("player_b", rng.integers(0, 5, b.nS).astype(np.int8))
    calls = [lambda: b.value_iteration(THETA, GAMMA),
             lambda: b.policy_evaluation(np.zeros(b.nS, np.int32), THETA, GAMMA),
             lambda: b.policy_improvement(np.zeros(b.nS), GAMMA),
             lambda: b.policy_iteration(np.zeros(b.nS, np.int32), THETA, GAMMA),
             lambda: b.policy_eval_dense(np.full((b.nS, 5), 0.2), THETA, GAMMA, k=3),
             lambda: b.modified_policy_iteration(5, THETA, GAMMA)]
    for call in calls:
        with pytest.raises(AssertionError, match=r"too many states \(%d\)" % b.nS):
            call()
    # the planners consume no tick: as a two-player handle it steps like the oracle from the start
    b.set_policy("player_b", None)
    o = O.Oracle(w, h, 0.2, n=n, seed=5, autoreset=True)
    obs = b.alloc(n, np.uint16); rew = b.alloc(n, np.int8); term = b.alloc(n, np.uint8); trunc = b.alloc(n, np.uint8)
    aa = b.alloc(n, np.int8); ab = b.alloc(n, np.int8)
    b.reset(obs=obs)
    assert np.array_equal(obs.download(), o.reset())
    for _ in range(8):
        a = rng.integers(0, 5, size=(2, n), dtype=np.int8)
        aa.upload(a[0]); ab.upload(a[1])
        b.step_plain(aa, ab, obs, rew, term, trunc)
        c = o.step(a[0], a[1])
        assert np.array_equal(obs.download(), c["obs"]) and np.array_equal(rew.download(), c["reward"])
    b.close()


# ---- 3. a result does not depend on what earlier calls left in the handle ---------------------------------------------------
def _six(g, b):
    """name -> the six planners on handle b, each returning a tuple of arrays / counters"""
    return {
        "vi": lambda: b.value_iteration(THETA, GAMMA),
        "pe": lambda: b.policy_evaluation(g.pi, THETA, GAMMA),
        "imp": lambda: b.policy_improvement(g.V, GAMMA),
        "pi": lambda: b.policy_iteration(g.pi0, THETA, GAMMA, max_sweeps=PI_SWEEPS),
        "de": lambda: b.policy_eval_dense(g.policy, THETA, GAMMA),                  # init=None: from zeros
        "mpi": lambda: b.modified_policy_iteration(5, 1e-6, GAMMA),
    }


def _same_result(got, want, what):
    assert len(got) == len(want)
    for i, (x, y) in enumerate(zip(got, want)):
        if isinstance(x, np.ndarray):
            same_bits(x, y, "%s output %d" % (what, i))
        else:
            assert x == y, (what, i, x, y)


def test_results_do_not_depend_on_earlier_calls(game):
    g = game(*PITCHES[3])
    assert (g.w, g.h) == (8, 7)
    fresh = {}
    for name in _six(g, None):
        b = g.fresh()
        fresh[name] = _six(g, b)[name]()
        b.close()
    b = g.fresh()
    capped = [lambda: b.value_iteration(THETA, GAMMA, max_sweeps=3), lambda: b.policy_iteration(g.pi, THETA, GAMMA, max_sweeps=4),
              lambda: b.modified_policy_iteration(3, THETA, GAMMA, max_sweeps=6), lambda: b.policy_evaluation(g.pi0, THETA, GAMMA, max_sweeps=2),
              lambda: b.policy_eval_dense(g.policy, THETA, GAMMA, init=g.init.copy(), max_sweeps=2),
              lambda: b.value_iteration(THETA, GAMMA, max_sweeps=1)]
    # in the first order dense evaluation from zeros follows value iteration, which leaves a non-zero V behind
    for order in (["vi", "de", "mpi", "imp", "pi", "pe"], ["pe", "pi", "mpi", "de", "imp", "vi"]):
        for i, name in enumerate(order):
            with pytest.raises(RuntimeError, match="without converging"):
                capped[i]()
            _same_result(_six(g, b)[name](), fresh[name], "%s as call %d of %s" % (name, i, order))
    # another opponent and back: the lists are rebuilt, the bits return
    other = ((g.opponent.astype(np.int64) + 1) % 5).astype(np.int8)
    side = "player_a" if g.learner == "player_b" else "player_b"
    b.set_policy(side, other)
    assert not np.array_equal(b.value_iteration(THETA, GAMMA)[1], fresh["vi"][1])
    b.set_policy(side, g.opponent)
    for name in ("de", "vi", "mpi"):
        _same_result(_six(g, b)[name](), fresh[name], name + " after set_policy and back")
    b.close()


def test_a_small_handle_after_a_large_one_matches_its_fixture(game):
    """the dynamic-LDS limit raised for 11x7 belongs to the function, not to the handle that raised it"""
    from gym_soccer_littman94_amd import SoccerSimultaneousEnv
    from gym_soccer_littman94_amd.planners import value_iteration
    g = game(*PITCHES[4])
    assert (g.w, g.h) == (11, 7)
    g.batch.value_iteration(THETA, GAMMA, max_sweeps=1000000)
    d = np.load(os.path.join(GOLD, "vi_5x4_s0p2_player_a_vs_random.npz"))
    env = SoccerSimultaneousEnv(width=5, height=4, slip_prob=float(d["slip"]), player_b_policy=d["policy"])
    pi, V, Q, cc = value_iteration(env, float(d["theta"]), float(d["discount_factor"]))
    assert cc == int(d["iterations"])
    same_bits(V, d["V"], "V"); same_bits(Q, d["Q"], "Q"); same_bits(pi, d["pi"], "pi")


# ---- 4. the cap -------------------------------------------------------------------------------------------------------------
def _e_state():
    text = open(os.path.join(ROOT, "include", "soccer_hip.h")).read()
    return int(re.search(r"#define\s+SOCCER_E_STATE\s+(-?\d+)", text).group(1))


def _raw(b, name, *args):
    """a planner through the C ABI: (return code, V, Q, pi, counter); outputs the call does not have stay zero"""
    nS = b.nS
    V = np.zeros(nS); Q = np.zeros((nS, 5)); pi = np.zeros(nS, np.int32); it = C.c_int32(-1)
    f = getattr(b.lib, name)
    if name == "soccer_value_iteration":
        theta, gamma, cap = args
        rc = f(b.h, theta, gamma, cap, V.ctypes.data, Q.ctypes.data, pi.ctypes.data, C.byref(it))
    elif name == "soccer_policy_evaluation":
        p, theta, gamma, cap = args
        p = np.ascontiguousarray(p, np.int32)
        rc = f(b.h, p.ctypes.data, theta, gamma, cap, V.ctypes.data, C.byref(it))
    elif name == "soccer_policy_iteration":
        p, theta, gamma, cap = args
        p = np.ascontiguousarray(p, np.int32)
        rc = f(b.h, p.ctypes.data, theta, gamma, cap, V.ctypes.data, Q.ctypes.data, pi.ctypes.data, C.byref(it))
    elif name == "soccer_policy_eval_dense":
        policy, k, theta, gamma, cap, init = args
        policy = np.ascontiguousarray(policy, np.float64); init = np.ascontiguousarray(init, np.float64)
        rc = f(b.h, policy.ctypes.data, k, theta, gamma, cap, init.ctypes.data, V.ctypes.data, C.byref(it))
    else:
        k, theta, gamma, cap = args
        rc = f(b.h, k, theta, gamma, cap, V.ctypes.data, Q.ctypes.data, pi.ctypes.data, C.byref(it))
    return rc, V, Q, pi.astype(np.int64), it.value


def _cap_cases(g):
    """(what, C call and its arguments, the Python call that must raise, the restatement's capped Plan)"""
    b = g.batch
    full_pi = g.want("pi", lambda: pn.policy_iteration(g.lists, g.pi0, THETA, GAMMA, max_sweeps=PI_SWEEPS))
    assert not full_pi.capped
    late = full_pi.sweeps - 1                                   # inside policy iteration's last evaluation
    return [
        ("value iteration", ("soccer_value_iteration", THETA, GAMMA, 5), lambda: b.value_iteration(THETA, GAMMA, max_sweeps=5),
         pn.value_iteration(g.lists, THETA, GAMMA, max_sweeps=5)),
        ("policy evaluation", ("soccer_policy_evaluation", g.pi, THETA, GAMMA, 5), lambda: b.policy_evaluation(g.pi, THETA, GAMMA, max_sweeps=5),
         pn.policy_evaluation(g.lists, g.pi, THETA, GAMMA, max_sweeps=5)),
        ("policy iteration, first evaluation", ("soccer_policy_iteration", g.pi0, THETA, GAMMA, 3),
         lambda: b.policy_iteration(g.pi0, THETA, GAMMA, max_sweeps=3), pn.policy_iteration(g.lists, g.pi0, THETA, GAMMA, max_sweeps=3)),
        ("policy iteration, last evaluation", ("soccer_policy_iteration", g.pi0, THETA, GAMMA, late),
         lambda: b.policy_iteration(g.pi0, THETA, GAMMA, max_sweeps=late), pn.policy_iteration(g.lists, g.pi0, THETA, GAMMA, max_sweeps=late)),
        ("dense evaluation", ("soccer_policy_eval_dense", g.policy, 7, THETA, GAMMA, 4, g.init),
         lambda: b.policy_eval_dense(g.policy, THETA, GAMMA, k=7, init=g.init.copy(), max_sweeps=4),
         pn.policy_eval_dense(g.rows, g.policy, THETA, GAMMA, k=7, init=g.init, max_sweeps=4)),
        ("dense evaluation, the k-th sweep", ("soccer_policy_eval_dense", g.policy, 7, THETA, GAMMA, 7, g.init),
         lambda: b.policy_eval_dense(g.policy, THETA, GAMMA, k=7, init=g.init.copy(), max_sweeps=7),
         pn.policy_eval_dense(g.rows, g.policy, THETA, GAMMA, k=7, init=g.init, max_sweeps=7)),
        ("modified policy iteration, a greedy step", ("soccer_modified_policy_iteration", 2, THETA, GAMMA, 4),
         lambda: b.modified_policy_iteration(2, THETA, GAMMA, max_sweeps=4), pn.modified_policy_iteration(g.rows, 2, THETA, GAMMA, max_sweeps=4)),
        ("modified policy iteration, an evaluation", ("soccer_modified_policy_iteration", 2, THETA, GAMMA, 5),
         lambda: b.modified_policy_iteration(2, THETA, GAMMA, max_sweeps=5), pn.modified_policy_iteration(g.rows, 2, THETA, GAMMA, max_sweeps=5)),
    ]


@pytest.mark.parametrize("w,h,slip,learner", [PITCHES[1], PITCHES[3]], ids=[IDS[1], IDS[3]])
def test_the_cap_returns_e_state_and_the_outputs_the_header_describes(w, h, slip, learner, game):
    g = game(w, h, slip, learner)
    for what, raw, call, want in _cap_cases(g):
        assert want.capped, what
        with pytest.raises(RuntimeError, match="without converging"):
            call()
        rc, V, Q, pi, counter = _raw(g.batch, *raw)
        assert rc == _e_state(), (what, rc)
        assert counter == want.counter, (what, counter, want.counter)
        same_bits(V, want.V, what + ": V")
        if want.Q is not None:
            same_bits(Q, want.Q, what + ": Q"); same_bits(pi, want.pi, what + ": pi")


# ---- 5. the dense lists are the ones the dense rows gave ---------------------------------------------------------------------
def test_dense_outputs_on_7x5_are_the_recorded_bits():
    """tests/golden/planner_dense_7x5_s0p3.npz holds the device's outputs from the build that still scanned full dense rows"""
    d = np.load(os.path.join(GOLD, "planner_dense_7x5_s0p3.npz"))
    b = SoccerBatch(1, 7, 5, 0.3)
    b.set_policy("player_a", d["opponent"])
    v, cc = b.policy_eval_dense(d["de_policy"], THETA, GAMMA, k=7, init=d["de_init"].copy())
    assert cc == int(d["de7_cc"])
    same_bits(v, d["de7_v"], "de7_v")
    v, cc = b.policy_eval_dense(d["de_policy"], THETA, GAMMA)
    assert cc == int(d["de0_cc"])
    same_bits(v, d["de0_v"], "de0_v")
    for tag, (k, theta) in zip(("mpi1", "mpi5", "mpi7"), MPI):
        pi, V, Q, counter = b.modified_policy_iteration(k, theta, GAMMA)
        assert counter == int(d[tag + "_counter"]), tag
        same_bits(V, d[tag + "_V"], tag + "_V"); same_bits(Q, d[tag + "_Q"], tag + "_Q"); same_bits(pi, d[tag + "_pi"].astype(np.int64), tag + "_pi")
    b.close()


# ---- 6. host memory ----------------------------------------------------------------------------------------------------------
_PEAK_CHILD = """
import resource, sys
import numpy as np
sys.path.insert(0, %r)
from gym_soccer_littman94_amd import SoccerBatch

def peaks():
    hwm = [int(line.split()[1]) for line in open("/proc/self/status") if line.startswith("VmHWM:")][0]
    return hwm, resource.getrusage(resource.RUSAGE_SELF).ru_maxrss

b = SoccerBatch(1, 11, 7, 0.2)
b.set_policy("player_b", np.random.default_rng(0).integers(0, 5, b.nS).astype(np.int8))
before = peaks()
cc = b.value_iteration(1e-8, 0.9)[3]
after = peaks()
b.close()
print("PEAK_KIB", before[0], after[0], before[1], after[1], cc)
"""


def test_first_planner_call_on_11x7_stays_under_1_gib_of_host_memory():
    """The transition export is about 0.2 GB (twice that if staged) and the lists about 20 MB; full dense rows of Pmat for
    every (s, a) were nS^2 * 40 bytes = 5.5 GB on top.  Peak resident set of a fresh process, before and after the call.
    ru_maxrss survives fork and exec, so the child starts at the peak of the process that started it and its growth there
    is max(parent's peak, own peak after) - max(parent's peak, own peak before): never more than the growth of the child's
    own high-water mark, VmHWM of /proc/self/status, which begins again at exec.  Both growths are bounded; the second is
    the one that does not depend on what ran earlier in the parent."""
    out = subprocess.run([sys.executable, "-c", _PEAK_CHILD % ROOT], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    hwm0, hwm1, ru0, ru1, cc = (int(x) for x in re.search(r"PEAK_KIB (\d+) (\d+) (\d+) (\d+) (\d+)", out.stdout).groups())
    growth, ru_growth = (hwm1 - hwm0) * 1024, (ru1 - ru0) * 1024    # both in KiB on Linux
    print("VmHWM before %.1f MiB, after %.1f MiB, growth %.1f MiB; ru_maxrss before %.1f MiB, after %.1f MiB, growth %.1f MiB; %d sweeps"
          % (hwm0 / 1024, hwm1 / 1024, growth / 2 ** 20, ru0 / 1024, ru1 / 1024, ru_growth / 2 ** 20, cc))
    assert cc > 20
    assert growth < 2 ** 30, "value_iteration grew the process's peak resident set by %.2f GiB" % (growth / 2 ** 30)
    assert ru_growth < 2 ** 30
