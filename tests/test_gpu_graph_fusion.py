"""Captured steps that are recorded as one multi-step launch (include/soccer_hip.h, "Deferred steps"): a run of consecutive
captured batched_step calls whose rows are evenly spaced is one rollout.  Whatever the library makes of a captured sequence,
every output, the state, the tick, the histogram and the sticky flags must be what one launch per call gives — against the
oracle, and bit for bit against a handle created with SOCCER_GRAPH_FUSE=0.  graph_info says how a capture was recorded.

Every case: 260 lanes (two workgroups, the second one ragged), lane_offset 8, 11 steps captured right after reset() — the
run starts at tick 1 and crosses an 8-tick Philox block — and every graph is replayed twice, so that the second replay
starts at tick 12, at another nibble phase."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gym_soccer_littman94_amd import SoccerBatch
from oracle.oracle import Oracle

N, T, OFF, SEED = 260, 11, 8, 7
KEYS = ("obs", "reward", "terminated", "truncated")


def _batch(monkeypatch, env=None, n=N, w=5, h=4, slip=0.0, **kw):
    """a handle created with `env` in the environment (the library reads its switches in soccer_create)"""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    kw.setdefault("autoreset", True); kw.setdefault("step_stats", False)
    b = SoccerBatch(n, w, h, slip, seed=SEED, lane_offset=OFF, **kw)
    for k in (env or {}):
        monkeypatch.delenv(k)
    return b


def _oracle(n=N, w=5, h=4, slip=0.0, autoreset=True):
    return Oracle(w, h, slip, n=n, seed=SEED, lane_offset=OFF, autoreset=autoreset)


def _state_equal(b, o):
    s = b.get_state()
    for k, v in (("row_a", o.row_a), ("col_a", o.col_a), ("row_b", o.row_b), ("col_b", o.col_b), ("poss", o.poss & 1),
                 ("needs_reset", (o.poss >> 1) & 1), ("t", o.t)):
        np.testing.assert_array_equal(s[k], v, err_msg=k)


class _Traj:
    """[rows][n] action and result blocks of one handle; row k of every block belongs to step k"""

    def __init__(self, b, acts, rows=None):
        self.b, self.acts, self.n = b, acts, b.n
        rows = rows or acts.shape[0]
        self.A = b.alloc((acts.shape[0], b.n), np.int8).upload(acts[:, 0])
        self.B = b.alloc((acts.shape[0], b.n), np.int8).upload(acts[:, 1])
        self.out = {"obs": b.alloc((rows, b.n), np.uint16), "reward": b.alloc((rows, b.n), np.int8),
                    "terminated": b.alloc((rows, b.n), np.uint8), "truncated": b.alloc((rows, b.n), np.uint8)}

    def step(self, k, out_row=None, obs=True):
        r = k if out_row is None else out_row
        o = self.out
        self.b.step_plain(self.A.row(k), self.B.row(k), o["obs"].row(r) if obs else None, o["reward"].row(r),
                          o["terminated"].row(r), o["truncated"].row(r))

    def download(self):
        return {k: v.download() for k, v in self.out.items()}

    def expect(self, o, ks, out_rows=None, skip_obs=()):
        """the oracle takes steps `ks`; the rows they wrote must hold its results"""
        got = self.download()
        for i, k in enumerate(ks):
            c = o.step(self.acts[k, 0], self.acts[k, 1])
            r = k if out_rows is None else out_rows[i]
            for key in KEYS:
                if key == "obs" and k in skip_obs:
                    continue
                np.testing.assert_array_equal(got[key][r], c[key], err_msg="%s of step %d" % (key, k))


def _acts(n=N, rows=T, seed=11):
    return np.random.default_rng(seed).integers(0, 5, size=(rows, 2, n), dtype=np.int8)


def _finish(b, o, hist=None, misuse=0):
    _state_equal(b, o)
    got_hist, got_misuse = b.stats()
    assert b.tick == o.tick and got_misuse == misuse
    if hist is not None:
        np.testing.assert_array_equal(got_hist, hist)
    b.close()


@pytest.mark.parametrize("wide", [False, True], ids=["packed", "wide"])
@pytest.mark.parametrize("slip", [0.0, 0.2, 0.03])
@pytest.mark.parametrize("pitch", [(5, 4), (7, 5)], ids=["5x4", "7x5"])
def test_fused_run_equals_the_oracle(monkeypatch, pitch, slip, wide):
    w, h = pitch
    acts = _acts()
    for step_stats in (False, True):
        b = _batch(monkeypatch, {"SOCCER_STATE_LAYOUT": "wide"} if wide else None, w=w, h=h, slip=slip, step_stats=step_stats)
        assert b.state_streams() == (6 if wide else 3)
        o = _oracle(w=w, h=h, slip=slip)
        tr = _Traj(b, acts)
        b.reset(); o.reset()
        b.graph_begin()
        for k in range(T):
            tr.step(k)
        g = b.graph_end()
        assert b.graph_info(g) == {"kernel_nodes": 1, "steps_fused": T, "fused_launches": 1}
        for rep in range(2):
            b.graph_launch(g, 1)
            tr.expect(o, range(T))
        b.graph_destroy(g)
        assert o.hist.sum() > 0
        _finish(b, o, hist=o.hist if step_stats else np.zeros(3, np.uint64))


@pytest.mark.parametrize("slip", [0.0, 0.2])
def test_fused_run_has_the_bits_of_one_launch_per_step(monkeypatch, slip):
    acts = _acts()
    res = []
    for env, info in (({"SOCCER_GRAPH_FUSE": "0"}, {"kernel_nodes": T, "steps_fused": 0, "fused_launches": 0}),
                      (None, {"kernel_nodes": 1, "steps_fused": T, "fused_launches": 1})):
        b = _batch(monkeypatch, env, slip=slip)
        tr = _Traj(b, acts)
        b.reset()
        b.graph_begin()
        for k in range(T):
            tr.step(k)
        g = b.graph_end()
        assert b.graph_info(g) == info
        per_replay = []
        for rep in range(2):
            b.graph_launch(g, 1)
            per_replay.append(tr.download())
        res.append((per_replay, b.get_state(), b.tick, b.stats()))
        b.graph_destroy(g); b.close()
    (r0, s0, t0, st0), (r1, s1, t1, st1) = res
    for rep in range(2):
        for key in KEYS:
            np.testing.assert_array_equal(r0[rep][key], r1[rep][key], err_msg="%s, replay %d" % (key, rep))
    for key in s0:
        np.testing.assert_array_equal(s0[key], s1[key], err_msg=key)
    assert t0 == t1 == 1 + 2 * T and st0[1] == st1[1] == 0
    np.testing.assert_array_equal(st0[0], st1[0])


# ---- what ends a run: the results stay right and graph_info shows how the capture was recorded ---------------------------------
def _capture_and_check(b, o, tr, record, info, ks=range(T), out_rows=None, skip_obs=()):
    b.reset(); o.reset()
    b.graph_begin()
    record()
    g = b.graph_end()
    assert b.graph_info(g) == info
    for rep in range(2):
        b.graph_launch(g, 1)
        tr.expect(o, ks, out_rows, skip_obs)
    b.graph_destroy(g)
    _finish(b, o)


def test_a_stamp_splits_the_run(monkeypatch):
    b, o = _batch(monkeypatch), _oracle()
    tr = _Traj(b, _acts())

    def record():
        for k in range(T):
            if k == 4:
                b.stamp(2)
            tr.step(k)
    _capture_and_check(b, o, tr, record, {"kernel_nodes": 2, "steps_fused": T, "fused_launches": 2})


def test_a_row_off_the_stride_splits_the_run(monkeypatch):
    b, o = _batch(monkeypatch), _oracle()
    tr = _Traj(b, _acts(), rows=T + 1)
    out_rows = [T if k == 6 else k for k in range(T)]       # step 6 writes the spare row: steps 0..5, step 6, steps 7..10

    def record():
        for k in range(T):
            tr.step(k, out_row=out_rows[k])
    _capture_and_check(b, o, tr, record, {"kernel_nodes": 3, "steps_fused": T - 1, "fused_launches": 2}, out_rows=out_rows)


def test_a_step_without_obs_splits_the_run(monkeypatch):
    b, o = _batch(monkeypatch), _oracle()
    tr = _Traj(b, _acts())

    def record():
        for k in range(T):
            tr.step(k, obs=k != 5)
    _capture_and_check(b, o, tr, record, {"kernel_nodes": 3, "steps_fused": T - 1, "fused_launches": 2}, skip_obs=(5,))


def test_steps_on_the_same_buffers_are_not_a_run(monkeypatch):
    b, o = _batch(monkeypatch), _oracle()
    acts = _acts()
    acts[:] = acts[0]                                       # one action row, one result row, every step
    tr = _Traj(b, acts)
    b.reset(); o.reset()
    b.graph_begin()
    for k in range(T):
        tr.step(0)
    g = b.graph_end()
    assert b.graph_info(g) == {"kernel_nodes": T, "steps_fused": 0, "fused_launches": 0}
    for rep in range(2):
        b.graph_launch(g, 1)
        got = tr.download()
        for k in range(T):
            c = o.step(acts[0, 0], acts[0, 1])
        for key in KEYS:
            np.testing.assert_array_equal(got[key][0], c[key], err_msg=key)
    b.graph_destroy(g)
    _finish(b, o)


def test_action_rows_inside_the_result_block_are_not_a_run(monkeypatch):
    """player A's action rows are the even rows of the block whose odd rows take the rewards: evenly spaced, but a result
    stream's extent covers rows a later step reads"""
    b, o = _batch(monkeypatch), _oracle()
    acts = _acts()
    tr = _Traj(b, acts)
    X = b.alloc((2 * T, N), np.int8)
    img = np.zeros((2 * T, N), np.int8); img[0::2] = acts[:, 0]
    X.upload(img)
    stride2 = b.alloc((2 * T, N), np.int8)                 # the other byte streams at the same spacing
    img[0::2] = acts[:, 1]
    stride2.upload(img)
    obs2 = b.alloc((2 * T, N), np.uint16); te2 = b.alloc((2 * T, N), np.uint8); tu2 = b.alloc((2 * T, N), np.uint8)
    b.reset(); o.reset()
    b.graph_begin()
    for k in range(T):
        b.step_plain(X.row(2 * k), stride2.row(2 * k), obs2.row(2 * k), X.row(2 * k + 1), te2.row(2 * k), tu2.row(2 * k))
    g = b.graph_end()
    assert b.graph_info(g) == {"kernel_nodes": T, "steps_fused": 0, "fused_launches": 0}
    for rep in range(2):
        b.graph_launch(g, 1)
        O, R, TE, TU = obs2.download(), X.download(), te2.download(), tu2.download()
        for k in range(T):
            c = o.step(acts[k, 0], acts[k, 1])
            np.testing.assert_array_equal(O[2 * k], c["obs"]); np.testing.assert_array_equal(R[2 * k + 1], c["reward"])
            np.testing.assert_array_equal(TE[2 * k], c["terminated"]); np.testing.assert_array_equal(TU[2 * k], c["truncated"])
            np.testing.assert_array_equal(R[2 * k], acts[k, 0])
    b.graph_destroy(g)
    _finish(b, o)


def test_a_callers_stream_is_not_deferred(monkeypatch):
    import torch
    s = torch.cuda.Stream()
    b, o = _batch(monkeypatch, stream=s.cuda_stream), _oracle()
    tr = _Traj(b, _acts())
    _capture_and_check(b, o, tr, lambda: [tr.step(k) for k in range(T)], {"kernel_nodes": T, "steps_fused": 0, "fused_launches": 0})


def test_a_fixed_policy_handle_is_not_fused(monkeypatch):
    b, o = _batch(monkeypatch), _oracle()
    policy = np.random.default_rng(5).integers(0, 5, size=b.nS).astype(np.int8)
    b.set_policy("player_b", policy)
    acts = _acts()
    tr = _Traj(b, acts)
    b.reset(); cur = o.reset()
    b.graph_begin()
    for k in range(T):
        out = tr.out
        b.step_plain(tr.A.row(k), None, out["obs"].row(k), out["reward"].row(k), out["terminated"].row(k), out["truncated"].row(k))
    g = b.graph_end()
    assert b.graph_info(g) == {"kernel_nodes": T, "steps_fused": 0, "fused_launches": 0}
    for rep in range(2):
        b.graph_launch(g, 1)
        got = tr.download()
        for k in range(T):
            c = o.step(acts[k, 0], policy[cur])
            for key in KEYS:
                np.testing.assert_array_equal(got[key][k], c[key], err_msg="%s of step %d" % (key, k))
            cur = c["obs"]
    b.graph_destroy(g)
    _finish(b, o)


def test_a_ragged_lane_count_is_not_fused(monkeypatch):
    n = 262
    b, o = _batch(monkeypatch, n=n), _oracle(n=n)
    tr = _Traj(b, _acts(n=n))
    # (rows of 262 bytes: the six even rows are dword-aligned and take the byte-parallel kernel over 260 lanes plus the per-lane
    # kernel over the last two, the five odd rows start 2 bytes off and take the per-lane kernel alone)
    _capture_and_check(b, o, tr, lambda: [tr.step(k) for k in range(T)], {"kernel_nodes": 6 * 2 + 5, "steps_fused": 0, "fused_launches": 0})


# ---- lengths, interleaving, launch parts -------------------------------------------------------------------------------------
def test_captures_of_1_2_and_5_steps_between_eager_steps(monkeypatch):
    b, o = _batch(monkeypatch), _oracle()
    tr = _Traj(b, _acts())
    b.reset(); o.reset()
    graphs = {}
    for name, ks in (("g1", [0]), ("g2", [1, 2]), ("g5", [3, 4, 5, 6, 7])):
        b.graph_begin()
        for k in ks:
            tr.step(k)
        graphs[name] = (b.graph_end(), ks)
        L = len(ks)
        assert b.graph_info(graphs[name][0]) == {"kernel_nodes": 1, "steps_fused": L if L > 1 else 0, "fused_launches": 1 if L > 1 else 0}
    for rep in range(2):
        for name in ("g1", "g5", "g2", "g5", "g1", "g2"):
            g, ks = graphs[name]
            b.graph_launch(g, 1); tr.expect(o, ks)
            tr.step(9); tr.expect(o, [9])                   # an eager step in between
            assert b.tick == o.tick
        g, ks = graphs["g5"]
        b.graph_launch(g, 2); b.sync()                      # two replays back to back: only the second one's rows are left
        for k in ks:
            o.step(tr.acts[k, 0], tr.acts[k, 1])
        tr.expect(o, ks)
    for g, _ in graphs.values():
        b.graph_destroy(g)
    _finish(b, o)


def test_run_rollout_run(monkeypatch):
    b, o = _batch(monkeypatch), _oracle()
    tr = _Traj(b, _acts())

    def record():
        for k in range(4):
            tr.step(k)
        out = tr.out
        b.rollout(3, tr.A.row(4), tr.B.row(4), act_stride=N, obs=out["obs"].row(4), reward=out["reward"].row(4),
                  terminated=out["terminated"].row(4), truncated=out["truncated"].row(4), out_stride=N)
        for k in range(7, T):
            tr.step(k)
    _capture_and_check(b, o, tr, record, {"kernel_nodes": 3, "steps_fused": 8, "fused_launches": 2})


@pytest.mark.parametrize("slip", [0.0, 0.2])
def test_fused_run_in_launch_parts(monkeypatch, slip):
    b, o = _batch(monkeypatch, {"SOCCER_SWAR_LAUNCH_LANES": "128"}, slip=slip), _oracle(slip=slip)
    tr = _Traj(b, _acts())
    # parts of 128, 128 and 4 lanes, every one over the same 11 ticks
    _capture_and_check(b, o, tr, lambda: [tr.step(k) for k in range(T)], {"kernel_nodes": 3, "steps_fused": T, "fused_launches": 1})


# ---- the sticky flags ----------------------------------------------------------------------------------------------------------
def _fused_and_unfused(monkeypatch, acts, **kw):
    res = []
    for env in ({"SOCCER_GRAPH_FUSE": "0"}, None):
        b = _batch(monkeypatch, env, **kw)
        tr = _Traj(b, acts)
        b.reset()
        b.graph_begin()
        for k in range(T):
            tr.step(k)
        g = b.graph_end()
        assert b.graph_info(g)["steps_fused"] == (0 if env else T)
        outs = []
        for rep in range(2):
            b.graph_launch(g, 1); outs.append(tr.download())
        res.append((outs, b.get_state(), b.tick, b.stats()[1]))
        b.graph_destroy(g); b.close()
    (o0, s0, t0, m0), (o1, s1, t1, m1) = res
    for rep in range(2):
        for key in KEYS:
            np.testing.assert_array_equal(o0[rep][key], o1[rep][key], err_msg="%s, replay %d" % (key, rep))
    for key in s0:
        np.testing.assert_array_equal(s0[key], s1[key], err_msg=key)
    assert t0 == t1 and m0 == m1
    return o1, m1


def test_a_bad_action_byte_in_a_fused_run(monkeypatch):
    acts = _acts()
    good = acts.copy(); good[3, 0, 17] = 0                  # NOOP, what a byte 7 executes as
    acts[3, 0, 17] = 7
    outs, misuse = _fused_and_unfused(monkeypatch, acts)
    assert misuse == SoccerBatch.MISUSE_ACTION
    o = _oracle()                                           # the oracle with the NOOP in its place
    o.reset()
    for rep in range(2):
        for k in range(T):
            c = o.step(good[k, 0], good[k, 1])
            for key in KEYS:
                np.testing.assert_array_equal(outs[rep][key][k], c[key], err_msg="%s of step %d" % (key, k))


def test_a_frozen_lane_in_a_fused_run(monkeypatch):
    outs, misuse = _fused_and_unfused(monkeypatch, _acts(), autoreset=False)
    assert misuse == SoccerBatch.MISUSE_FROZEN
    assert outs[0]["terminated"].any()                      # a goal fell in the first replay; the lane was stepped again
