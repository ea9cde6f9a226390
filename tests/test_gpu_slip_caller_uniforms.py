"""batched_step_ex with caller-supplied uniforms on slip_prob > 0 handles in every shape of the byte-parallel step
(step_kernel_swar<OUT, SLIPM = 3, POLICY, GEO, true> + the one-workgroup exact walk of the groups it lists), against the oracle.

Every step: the step uniforms sit on the reference's own running sums of each lane's CURRENT list (Oracle.dump_table, looked up
by tuple and joint action), near them, on both sides of the 2^-40 margin or on special values; every output is filled with a
sentinel first (a listed group nobody writes must not pass on stale bytes); every lane of every output is compared.  At the end:
state, histogram, misuse and tick.  exact_walk_stats() shows that the listed path ran, and its group count is the one the CPU
build of the same decision (tests/host/swar_host.cpp: swar_listed_f64) predicts from the uniforms."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIALS = np.array([0.0, -0.0, 5e-324, 1.0 - 2.0 ** -53, 1.0, 1.0 + 2.0 ** -52, 7.0, -0.5, np.nan, np.inf, -np.inf])
REGIMES = ("random", "mixed", "every_lane", "margin", "special")


@pytest.fixture(scope="module")
def decide(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("slipgpu") / "libswar_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-o", so,
                           os.path.join(ROOT, "tests", "host", "swar_host.cpp")])
    L = C.CDLL(so)
    L.swar_listed_f64.argtypes = [C.c_double, C.c_long, C.c_void_p, C.c_void_p]

    def listed(slip, u):
        u = np.ascontiguousarray(u, np.float64)
        out = np.zeros(len(u) // 4, np.uint8)
        L.swar_listed_f64(float(slip), len(u), u.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        return out
    return listed


class Lists:
    """the reference's sequential running sums of every (tuple, joint action) list"""

    def __init__(self, o):
        rows, prob = o.dump_table()
        key = self._code(rows[:, :7].astype(np.int64))
        start = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
        self.m = np.diff(np.r_[start, len(rows)])
        self.key = key[start]
        assert np.all(np.diff(self.key) > 0)
        self.S = np.full((len(start), int(self.m.max())), np.inf)
        acc = np.zeros(len(start))
        for k in range(int(self.m.max())):
            sel = self.m > k
            acc[sel] = acc[sel] + prob[start[sel] + k]            # left to right, as categorical_sample's cumsum
            self.S[sel, k] = acc[sel]

    @staticmethod
    def _code(c):
        code = np.zeros(len(c), np.int64)
        for j in range(c.shape[1]):
            code = code * 32 + c[:, j]
        return code

    def sums(self, o, aa, ab):
        """S[lane, :] and m[lane] of each lane's current list (frozen lanes: whatever list their tuple has)"""
        c = self._code(np.stack([o.row_a, o.col_a, o.row_b, o.col_b, o.poss & 1, aa, ab], 1).astype(np.int64))
        i = np.minimum(np.searchsorted(self.key, c), len(self.key) - 1)
        found = self.key[i] == c
        assert np.all(found | ((o.poss >> 1) & 1).astype(bool))     # a frozen lane is not stepped: any list will do
        i = np.where(found, i, 0)
        return self.S[i], self.m[i]


def uniforms(rng, S, m, regime):
    n = len(m)
    k = (rng.random(n) * m).astype(np.int64)
    on = S[np.arange(n), k]
    side = rng.integers(0, 3, n)
    thr = np.where(side == 0, on, np.where(side == 1, np.nextafter(on, 0.0), np.nextafter(on, 2.0)))
    r = rng.random(n)
    if regime == "random":
        return r
    if regime == "mixed":
        return np.where(rng.random(n) < 0.3, thr, r)
    if regime == "every_lane":
        return thr
    if regime == "margin":
        d = 2.0 ** -40 * (1 + rng.choice([-1.0, 1.0], n) * 2.0 ** -20) * rng.choice([-1.0, 1.0], n)
        return np.where(rng.random(n) < 0.5, on + d, thr)
    return np.where(rng.random(n) < 0.5, SPECIALS[rng.integers(0, len(SPECIALS), n)], thr)


class Run:
    """one handle and its oracle, stepped together with every output checked"""

    def __init__(self, w, h, slip, n, out=2, autoreset=True, max_steps=100, seed=3, lane_offset=0, u_reset=True,
                 policy=None, stream_actions=False, decide=None):
        self.n, self.out, self.slip, self.autoreset, self.with_ur = n, out, slip, autoreset, u_reset
        self.b = SoccerBatch(n, w, h, slip, seed=seed, autoreset=autoreset, max_steps=max_steps, lane_offset=lane_offset,
                             step_stats=out == 2, stream_actions=stream_actions)
        self.o = Oracle(w, h, slip, n=n, seed=seed, autoreset=autoreset, max_steps=max_steps, lane_offset=lane_offset)
        self.lists = Lists(self.o)
        self.rng = np.random.default_rng(int(slip * 1000) + 7 * w + n + out)
        self.decide, self.predicted = decide, 0
        self.policy_side = None
        if policy is not None:
            self.policy_side, self.pol = policy, self.rng.integers(0, 5, self.b.nS).astype(np.int8)
            self.b.set_policy(policy, self.pol)
        b = self.b
        self.A = b.alloc(n, np.int8); self.B = b.alloc(n, np.int8); self.U = b.alloc(n, np.float64); self.UR = b.alloc(n, np.float64)
        self.obs = b.alloc(n, np.uint16); self.rew = b.alloc(n, np.int8); self.te = b.alloc(n, np.uint8); self.tr = b.alloc(n, np.uint8)
        self.code = b.alloc(n, np.uint8) if out == 2 else None
        self.fin = b.alloc(n, np.uint16) if out == 2 else None
        if out == 1:
            self.ra32 = b.alloc(n, np.float32); self.rb32 = b.alloc(n, np.float32); self.done = b.alloc(n, np.uint8)
            self.lr = b.alloc(n, np.int8).upload(np.zeros(n, np.int8)); self.lr_exp = np.zeros(n, np.int8)
        b.reset(obs=self.obs)
        self.obs_now = self.obs.download()
        np.testing.assert_array_equal(self.obs_now, self.o.reset())

    def outputs(self):
        d = dict(obs=self.obs, reward=self.rew, terminated=self.te, truncated=self.tr, prob_code=self.code, final_obs=self.fin)
        if self.out == 1:
            d.update(reward_a_f32=self.ra32, reward_b_f32=self.rb32, finished=self.done, last_return=self.lr)
        return d

    def prepare(self, regime, force=()):
        """actions and uniforms of the next step, uploaded; the sentinel in every output"""
        n, rng = self.n, self.rng
        a = rng.integers(0, 5, size=(2, n)).astype(np.int8)
        if self.policy_side is not None:
            a[0 if self.policy_side == "player_a" else 1] = self.pol[self.obs_now]
        S, m = self.lists.sums(self.o, a[0], a[1])
        u = uniforms(rng, S, m, regime)
        for lane in force:                                       # this lane exactly on a running sum of its list
            u[lane] = S[lane, 0]
        ur = rng.random(n) if self.with_ur else None
        self.A.upload(a[0]); self.B.upload(a[1]); self.U.upload(u)
        if ur is not None:
            self.UR.upload(ur)
        for k, buf in self.outputs().items():
            if buf is not None and k != "last_return":
                buf.fill(0xA5)
        return a, u, ur

    def launch(self):
        self.b.step(self.A, self.B, u_step=self.U, u_reset=self.UR if self.with_ur else None, **self.outputs())

    def check(self, a, u, ur, what, counted=True, first=0, count=None):
        """the oracle's step; counted: the step went through SLIPM = 3 over lanes [first, first + count)"""
        c = self.o.step(a[0], a[1], u_step=u, u_reset=ur)
        eq = np.testing.assert_array_equal
        eq(self.obs.download(), c["obs"], err_msg="obs " + what)
        rew = self.rew.download()
        eq(rew, c["reward"], err_msg="reward " + what)
        eq(self.te.download(), c["terminated"], err_msg="terminated " + what)
        eq(self.tr.download(), c["truncated"], err_msg="truncated " + what)
        done = (c["terminated"] | c["truncated"]).astype(np.uint8)
        if self.out == 2:
            eq(self.code.download(), c["prob_code"], err_msg="prob_code " + what)
            eq(self.fin.download(), c["final_obs"], err_msg="final_obs " + what)
        if self.out == 1:
            f = c["reward"].astype(np.float32)
            eq(self.ra32.download(), f, err_msg="reward_a_f32 " + what)
            eq(self.rb32.download(), np.float32(0.0) - f, err_msg="reward_b_f32 " + what)
            eq(self.done.download(), done, err_msg="finished " + what)
            assert self.autoreset
            self.lr_exp = np.where(done.astype(bool), c["reward"], self.lr_exp)     # A's return of the episode that just ended
            eq(self.lr.download(), self.lr_exp, err_msg="last_return " + what)
        self.obs_now = c["obs"]
        if counted and self.decide is not None:
            count = (self.n & ~3) - first if count is None else count
            self.predicted += int(self.decide(self.slip, u[first:first + count]).sum())
        return c

    def step(self, regime, what="", **kw):
        a, u, ur = self.prepare(regime)
        self.launch()
        return self.check(a, u, ur, "%s regime %s" % (what, regime), **kw)

    def finish(self, exact=True, misuse=0):
        b, o = self.b, self.o
        s = b.get_state()
        for k, v in (("row_a", o.row_a), ("col_a", o.col_a), ("row_b", o.row_b), ("col_b", o.col_b), ("poss", o.poss & 1),
                     ("needs_reset", (o.poss >> 1) & 1), ("t", o.t)):
            np.testing.assert_array_equal(s[k], v, err_msg=k)
        if self.out == 2:
            np.testing.assert_array_equal(b.stats()[0], o.hist)
        assert b.misuse() == misuse and b.tick == o.tick
        parts, groups = b.exact_walk_stats()
        assert parts > 0 and groups > 0, "the listed path (SLIPM = 3 + exact walk) did not run"
        if exact and self.decide is not None:
            assert groups == self.predicted, (groups, self.predicted)
        return parts, groups


def _close(r):
    r.b.close()


@pytest.mark.parametrize("out", [0, 1, 2])
@pytest.mark.parametrize("w,h,slip", [(5, 4, 0.2), (6, 4, 0.5), (7, 5, 0.3), (9, 6, 0.1), (11, 7, 0.2), (5, 4, 1.0),
                                      (7, 5, 0.9), (5, 4, 0.05)])
def test_every_regime_every_output_shape(decide, w, h, slip, out):
    r = Run(w, h, slip, 2048, out=out, decide=decide)
    for k, regime in enumerate(REGIMES + ("every_lane",)):
        r.step(regime, "step %d" % k)
    r.finish()
    _close(r)


@pytest.mark.parametrize("w,h,slip", [(5, 4, 0.2), (7, 5, 0.3), (5, 4, 1.0)])
def test_philox_reset_draws_next_to_caller_step_uniforms(decide, w, h, slip):
    """u_reset = NULL and max_steps = 5: listed groups hold lanes that truncate and reset on their Philox word"""
    r = Run(w, h, slip, 1024, out=2, max_steps=5, u_reset=False, decide=decide)
    for k in range(12):
        r.step(REGIMES[k % len(REGIMES)], "step %d" % k)
    r.finish()
    _close(r)


@pytest.mark.parametrize("w,h,slip", [(5, 4, 0.5), (9, 6, 0.1)])
def test_without_autoreset_frozen_lanes_and_masked_resets(decide, w, h, slip):
    """autoreset off: finished lanes stay frozen and are stepped anyway (misuse, left untouched), a masked reset revives some"""
    r = Run(w, h, slip, 1024, out=2, autoreset=False, max_steps=6, decide=decide)
    for k in range(14):
        r.step(REGIMES[k % len(REGIMES)], "step %d" % k)
        if k % 4 == 3:
            mask = (r.rng.random(r.n) < 0.5).astype(np.uint8)
            ur = r.rng.random(r.n)
            r.b.reset(mask=r.b.alloc(r.n, np.uint8).upload(mask), u_reset=r.b.alloc(r.n, np.float64).upload(ur), obs=r.obs)
            np.testing.assert_array_equal(r.obs.download(), r.o.reset(mask=mask, u_reset=ur))
            r.obs_now = r.obs.download()
    assert ((r.o.poss >> 1) & 1).any()
    r.finish(misuse=SoccerBatch.MISUSE_FROZEN)
    _close(r)


@pytest.mark.parametrize("side", ["player_a", "player_b"])
@pytest.mark.parametrize("w,h,slip", [(5, 4, 0.2), (7, 5, 0.9)])
def test_fixed_policy_side(decide, w, h, slip, side):
    r = Run(w, h, slip, 1024, out=2, policy=side, decide=decide)
    for k, regime in enumerate(REGIMES):
        r.step(regime, "step %d" % k)
    r.finish()
    _close(r)


@pytest.mark.parametrize("n", [4, 8, 8192 + 1, 8192 + 2, 8192 + 3])
def test_lane_counts_and_ragged_tails(decide, n):
    """the ragged tail (n % 4 lanes) takes the per-lane kernel next to a non-empty work list"""
    r = Run(5, 4, 0.2, n, out=2, decide=decide)
    for k, regime in enumerate(REGIMES + ("every_lane",)):
        r.step(regime, "step %d" % k)
    r.finish()
    _close(r)


def test_split_launch_parts_share_one_list(decide, monkeypatch):
    """SOCCER_SWAR_LAUNCH_LANES=4096: four launch parts per step, each followed by its own walk of the one list; listed groups
    sit in the first and the last group of every part"""
    monkeypatch.setenv("SOCCER_SWAR_LAUNCH_LANES", "4096")
    n = 3 * 4096 + 1028 + 2
    r = Run(7, 5, 0.3, n, out=2, decide=decide)
    n4 = n & ~3
    edges = [l for c0 in range(0, n4, 4096) for l in (c0, min(c0 + 4096, n4) - 4)]
    steps = 0
    for k, regime in enumerate(("random", "mixed", "every_lane", "random", "margin")):
        a, u, ur = r.prepare(regime, force=edges)
        r.launch()
        r.check(a, u, ur, "step %d regime %s" % (k, regime))
        listed = decide(r.slip, u[:n4])
        assert all(listed[e // 4] for e in edges)
        steps += 1
    parts, _ = r.finish()
    assert parts == 4 * steps
    _close(r)


def test_lane_offsets(decide):
    """lane_offset 2^20 + 4 keeps a thread's four lanes one Philox block (SLIPM = 3, here with Philox reset draws); 2^20 + 2 does
    not, and the whole step takes the per-lane kernel: the work list stays unused"""
    r = Run(5, 4, 0.2, 2048, out=2, lane_offset=2 ** 20 + 4, u_reset=False, max_steps=8, decide=decide)
    for k in range(10):
        r.step(REGIMES[k % len(REGIMES)], "step %d" % k)
    r.finish()
    _close(r)
    r = Run(5, 4, 0.2, 2048, out=2, lane_offset=2 ** 20 + 2, u_reset=False, max_steps=8)
    for k in range(6):
        r.step(REGIMES[k % len(REGIMES)], "step %d" % k)
    assert r.b.exact_walk_stats() == (0, 0)
    r.b.close()


def test_stream_actions(decide):
    r = Run(6, 4, 0.5, 2048, out=1, stream_actions=True, decide=decide)
    for k, regime in enumerate(REGIMES):
        r.step(regime, "step %d" % k)
    r.finish()
    _close(r)


def test_graph_captured_before_the_work_list_exists(decide):
    """the first u-step call of a fresh handle is a capture: no work list can be allocated inside it, so the graph holds the
    per-lane kernel; replays stay exact, and the eager calls after them take SLIPM = 3"""
    r = Run(5, 4, 0.3, 2048, out=2, decide=decide)
    a, u, ur = r.prepare("every_lane")
    r.b.graph_begin(); r.launch(); g = r.b.graph_end()
    r.b.graph_launch(g, 1)
    r.check(a, u, ur, "first replay", counted=False)
    for k in range(4):
        a, u, ur = r.prepare(REGIMES[k])
        r.b.graph_launch(g, 1)
        r.check(a, u, ur, "replay %d" % k, counted=False)
    assert r.b.exact_walk_stats() == (0, 0)
    for k, regime in enumerate(REGIMES):
        r.step(regime, "eager %d" % k)
    r.finish()
    r.b.graph_destroy(g)
    _close(r)


def test_graph_replays_with_every_lane_listed(decide):
    r = Run(7, 5, 0.2, 2048, out=1, decide=decide)
    for k in range(2):
        r.step("mixed", "eager %d" % k)
    r.b.graph_begin(); r.launch(); g = r.b.graph_end()
    for k in range(20):
        a, u, ur = r.prepare("every_lane")
        r.b.graph_launch(g, 1)
        r.check(a, u, ur, "replay %d" % k)
    parts, groups = r.finish()
    assert parts == 22 and groups > 20 * (2048 // 4) // 2
    r.b.graph_destroy(g)
    _close(r)


def test_graph_of_three_steps(decide):
    """three consecutive steps in one graph: three tails, each consuming the list the step before it filled"""
    r = Run(5, 4, 0.2, 2048, out=2, decide=decide)
    r.step("mixed", "eager")
    bufs = [(r.b.alloc(r.n, np.int8), r.b.alloc(r.n, np.int8), r.b.alloc(r.n, np.float64), r.b.alloc(r.n, np.float64)) for _ in range(3)]
    r.b.graph_begin()
    for (A, B, U, UR) in bufs:
        r.b.step(A, B, u_step=U, u_reset=UR, **r.outputs())
    g = r.b.graph_end()
    for rep in range(4):
        # the three steps' inputs are chosen one after the other from the oracle's state, which the oracle then takes
        plans = []
        for j, (A, B, U, UR) in enumerate(bufs):
            a = r.rng.integers(0, 5, size=(2, r.n)).astype(np.int8)
            S, m = r.lists.sums(r.o, a[0], a[1])
            u = uniforms(r.rng, S, m, ("every_lane", "mixed", "margin")[j]); ur = r.rng.random(r.n)
            A.upload(a[0]); B.upload(a[1]); U.upload(u); UR.upload(ur)
            c = r.o.step(a[0], a[1], u_step=u, u_reset=ur)
            r.predicted += int(decide(r.slip, u).sum())
            plans.append(c)
        for buf in (r.obs, r.rew, r.te, r.tr, r.code, r.fin):
            buf.fill(0xA5)
        r.b.graph_launch(g, 1)
        c = plans[-1]
        np.testing.assert_array_equal(r.obs.download(), c["obs"], err_msg="obs, replay %d" % rep)
        np.testing.assert_array_equal(r.rew.download(), c["reward"])
        np.testing.assert_array_equal(r.te.download(), c["terminated"]); np.testing.assert_array_equal(r.tr.download(), c["truncated"])
        np.testing.assert_array_equal(r.code.download(), c["prob_code"]); np.testing.assert_array_equal(r.fin.download(), c["final_obs"])
    parts, _ = r.finish()
    assert parts == 1 + 3 * 4
    r.b.graph_destroy(g)
    _close(r)
