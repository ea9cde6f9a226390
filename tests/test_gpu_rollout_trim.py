"""The stream rollout's step loop in step form (csrc/soccer_swar.hpp: swar::Carry4; csrc/soccer_rollout_kernels.hpp: the
carried step, the hoisted byte tables, the shape of a captured run whose statistics nobody reads) held to the CPU oracle —
not to the eager step, whose kernel shares the step's body.

Main grid: 3 080 lanes (three full workgroups and a partial one), three eager steps, then a captured run of 19: ticks
3 .. 21 start on an odd tick and cross two eight-tick block boundaries.  Pitches 5x4 and 6x6 (byte tables), 7x5 (arithmetic,
packed state) and 15x4 (arithmetic, six state streams); slip 0, 0.2 (selection by table) and 0.03 (one by one); episodes of
100 steps and of 3 (a reset in almost every block); with and without step statistics."""
import os
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch
from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_graph_fusion import KEYS, _Traj, _state_equal  # noqa: E402
from test_gpu_swar import _rollout_vs_oracle  # noqa: E402
from test_gpu_rollout_action_sources import _fixed_policy, _threshold_rows  # noqa: E402

pytestmark = pytest.mark.gpu

N, EAGER, RUN, OFF, SEED = 3080, 3, 19, 8, 7
ROWS = EAGER + RUN
PITCHES = [(5, 4), (6, 6), (7, 5), (15, 4)]
FUSED = {"kernel_nodes": 1, "steps_fused": RUN, "fused_launches": 1}


def _pair(monkeypatch, w, h, slip, max_steps=100, step_stats=False, env=None):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)                            # the library reads its switches in soccer_create
    b = SoccerBatch(N, w, h, slip, seed=SEED, lane_offset=OFF, autoreset=True, max_steps=max_steps, step_stats=step_stats)
    for k in (env or {}):
        monkeypatch.delenv(k)
    return b, Oracle(w, h, slip, n=N, seed=SEED, lane_offset=OFF, autoreset=True, max_steps=max_steps)


def _acts(seed=11):
    return np.random.default_rng(seed).integers(0, 5, size=(ROWS, 2, N), dtype=np.int8)


def _eager_then_run(b, tr, info=FUSED):
    """reset, three eager steps, the other 19 captured and replayed once -> the histogram as it stood before the replay"""
    b.reset()
    for k in range(EAGER):
        tr.step(k)
    before = b.stats()[0].copy()
    b.graph_begin()
    for k in range(EAGER, ROWS):
        tr.step(k)
    g = b.graph_end()
    assert b.graph_info(g) == info
    b.graph_launch(g, 1)
    b.graph_destroy(g)
    return before


def _check_case(monkeypatch, w, h, slip, max_steps, step_stats, env=None, info=FUSED):
    b, o = _pair(monkeypatch, w, h, slip, max_steps, step_stats, env)
    tr = _Traj(b, _acts())
    o.reset()
    before = _eager_then_run(b, tr, info)
    tr.expect(o, range(ROWS))                               # the four streams of all 22 steps
    _state_equal(b, o)
    hist, misuse = b.stats()
    assert b.tick == o.tick and misuse == 0 and o.hist.sum() > 0
    if step_stats:
        np.testing.assert_array_equal(hist, o.hist)
    else:
        np.testing.assert_array_equal(hist, before)         # nothing reads a run's statistics: nothing counts them
        np.testing.assert_array_equal(hist, np.zeros(3, np.uint64))
    b.close()


@pytest.mark.parametrize("max_steps", [100, 3])
@pytest.mark.parametrize("slip", [0.0, 0.2, 0.03])
@pytest.mark.parametrize("pitch", PITCHES, ids=["%dx%d" % p for p in PITCHES])
def test_captured_run_after_eager_steps_equals_the_oracle(monkeypatch, pitch, slip, max_steps):
    for step_stats in (True, False):
        _check_case(monkeypatch, pitch[0], pitch[1], slip, max_steps, step_stats)


@pytest.mark.parametrize("step_stats", [True, False])
@pytest.mark.parametrize("slip", [0.0, 0.2])
def test_captured_run_in_launch_parts(monkeypatch, slip, step_stats):
    # parts of 1 024, 1 024, 1 024 and 8 lanes, every one over the same 19 ticks
    _check_case(monkeypatch, 5, 4, slip, 3, step_stats, env={"SOCCER_SWAR_LAUNCH_LANES": "1024"},
                info={"kernel_nodes": 4, "steps_fused": RUN, "fused_launches": 1})


@pytest.mark.parametrize("pitch,slip", [((5, 4), 0.0), ((5, 4), 0.2), ((7, 5), 0.0), ((15, 4), 0.03)])
def test_one_launch_per_step_gives_identical_bytes(monkeypatch, pitch, slip):
    res = []
    for env, info in (({"SOCCER_GRAPH_FUSE": "0"}, {"kernel_nodes": RUN, "steps_fused": 0, "fused_launches": 0}), (None, FUSED)):
        b, _ = _pair(monkeypatch, pitch[0], pitch[1], slip, 3, env=env)
        tr = _Traj(b, _acts())
        _eager_then_run(b, tr, info)
        res.append((tr.download(), b.get_state(), b.tick, b.stats()))
        b.close()
    (r0, s0, t0, st0), (r1, s1, t1, st1) = res
    for key in KEYS:
        np.testing.assert_array_equal(r0[key], r1[key], err_msg=key)
    for key in s0:
        np.testing.assert_array_equal(s0[key], s1[key], err_msg=key)
    assert t0 == t1 == 1 + ROWS and st0[1] == st1[1] == 0
    np.testing.assert_array_equal(st0[0], st1[0])


@pytest.mark.parametrize("pitch,slip", [((5, 4), 0.0), ((5, 4), 0.2), ((7, 5), 0.0)])
@pytest.mark.parametrize("byte", [7, 0x85])
def test_a_bad_action_byte_in_step_7_of_the_run(monkeypatch, pitch, slip, byte):
    acts = _acts()
    lane, row = 1029, EAGER + 7
    b, o = _pair(monkeypatch, pitch[0], pitch[1], slip)
    tr = _Traj(b, acts)
    tr.B.upload_rows(row, np.where(np.arange(N) == lane, byte, acts[row, 1]).astype(np.uint8).view(np.int8)[None])
    o.reset()
    _eager_then_run(b, tr)
    assert b.misuse() == SoccerBatch.MISUSE_ACTION
    # the groups without the byte, against the oracle: before step 7 every lane; from it on every lane but the byte's group
    # (what it executes as is checked exhaustively on the CPU, tests/test_swar_carry_host.py)
    got = tr.download()
    clean = np.ones(N, bool); clean[lane & ~3:(lane & ~3) + 4] = False
    for k in range(ROWS):
        c = o.step(acts[k, 0], acts[k, 1])
        sel = clean if k >= row else np.ones(N, bool)
        for key in KEYS:
            np.testing.assert_array_equal(got[key][k][sel], c[key][sel], err_msg="%s of step %d" % (key, k))
    b.close()


@pytest.mark.parametrize("max_steps", [100, 3])
@pytest.mark.parametrize("slip", [0.0, 0.2, 0.03])
@pytest.mark.parametrize("pitch", PITCHES, ids=["%dx%d" % p for p in PITCHES])
def test_batched_rollout_of_19_steps_always_counts(monkeypatch, pitch, slip, max_steps):
    """batched_rollout and batched_rollout_ex (final_obs / prob_code) on the same handles: trajectories, final_obs / prob_code,
    return_sum, episode_count and the histogram (also on a handle without step statistics) against the oracle"""
    acts = _acts(seed=13)[:RUN]
    for step_stats in (True, False):
        b, o = _pair(monkeypatch, pitch[0], pitch[1], slip, max_steps, step_stats)
        b.reset(); o.reset()
        for extras in (False, True):
            _rollout_vs_oracle(b, o, acts, RUN, N, extras=extras, strict=True)      # the state carries over: ticks 1 .. 19, 20 .. 38
        assert o.hist.sum() > 0
        b.close()


def test_self_play_and_fixed_policy_rollouts_share_the_body(monkeypatch):
    """config 5 (both sides sampled from mixed-policy rows) and a fixed policy against a streamed side, 5x4: the oracle is given
    the kernel's own draws (Oracle.sample_actions_mixed), as tests/test_gpu_rollout_action_sources.py does it"""
    rng = np.random.default_rng(3)
    b, o = _pair(monkeypatch, 5, 4, 0.0, step_stats=True)
    b.reset(); o.reset()
    _rollout_vs_oracle(b, o, None, RUN, N, sample=True, mix=(_threshold_rows(rng, o.nS), _threshold_rows(rng, o.nS)), extras=False, strict=True)
    assert b.rollout_shape()["action_source"] == 2
    b.close()
    b, o = _pair(monkeypatch, 5, 4, 0.2, step_stats=True)
    policy = _fixed_policy(rng, o.nS)
    b.set_policy("player_a", policy)
    b.reset(); o.reset()
    _rollout_vs_oracle(b, o, _acts(seed=17)[:RUN], RUN, N, policy=policy, fixed="player_a", extras=False, strict=True)
    assert b.rollout_shape()["action_source"] == 4
    b.close()
