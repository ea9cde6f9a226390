"""-m gpu: the environment's own kernels on the pitches at every boundary of their dispatch (tests/large_pitch_cases.py) — the last
pitch on the byte tables and its first arithmetic neighbours, the corner of the packed state (row 7, column 15), byte-parallel
kernels on handles whose six streams are theirs by nature (rows to 17, columns to 31), per-lane kernels with the observation
table in LDS up to 152 064 B and in global memory, observation indices with the top bit set, and the largest pitches Rules::build
accepts next to the ones it refuses.  Everything is bit for bit against the CPU oracle; there are no tolerances.
tests/test_pitch_boundaries_np.py shows without a GPU that the oracle's side of every case reaches what the case is for.

(a) one step from every live and goal tuple x 25 action pairs, (b) rollouts of every action source, (c) resets, (d) acceptance
and refusal; the last test asserts what the cases together reached."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch, _lib
from oracle.oracle import Oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import large_pitch_cases as lp  # noqa: E402
from large_pitch_cases import CASES, MAX_STEPS, N, NAMES, SLIPS, STRIDE, T  # noqa: E402
from test_gpu_rollout_action_sources import (BYTE_PARALLEL, GLOBAL, NONE, PER_LANE, SLIP_ROWS_BYTES, SOURCES, STAGING_BYTES,  # noqa: E402
                                             _check_shape, _fixed_policy, _threshold_rows)
from test_gpu_state_layout import _IO as _ShiftedIO  # noqa: E402
from test_gpu_swar import _IO, _check, _rollout_vs_oracle, _state_equal  # noqa: E402

pytestmark = pytest.mark.gpu

SEED, TICK0 = 1994, 8 * 1000 + 3        # the sweeps all step on this tick (slip 0: the fourth tick of a Philox block)
_REACHED = {}                           # name -> what its tests saw (test_zz_the_cases_reached_every_placement)


def _reached(name):
    return _REACHED.setdefault(name, dict(kernels=set(), streams=set(), small=set(), lut_lds=set(), per_lane_lds=set()))


def _set_tick(b, tick):
    b._check(b.lib.soccer_set_tick(b.h, tick))


# ---- (a) the whole transition relation, one step --------------------------------------------------------------------------------
_SWEEP = {}


def _sweep(name, slip):
    """the sweep's lanes and an oracle of that many, made once per (case, slip); one case is kept at a time"""
    key = (name, slip)
    if key not in _SWEEP:
        for k in [k for k in _SWEEP if k[0] != name]:
            del _SWEEP[k]
        c = CASES[name]
        tup = lp.tuples_of(Oracle(c["w"], c["h"], slip, n=1), [1, 2])
        st, aa, ab = lp.sweep_lanes(tup)
        o = Oracle(c["w"], c["h"], slip, n=len(st), seed=SEED, autoreset=True, max_steps=MAX_STEPS)
        _SWEEP[key] = dict(o=o, st=st, aa=aa, ab=ab, n=len(st))
        _inject(o, _SWEEP[key], 0)
        _SWEEP[key]["cur"] = lp.observations(o)                 # the observation every lane starts from; 0 on the goal tuples
    return _SWEEP[key]


def _inject(x, s, t):
    st = s["st"]
    x.set_state(st[:, 0].astype(np.int8), st[:, 1].astype(np.int8), st[:, 2].astype(np.int8), st[:, 3].astype(np.int8), st[:, 4].astype(np.uint8),
                t=np.full(s["n"], t, np.uint8), needs_reset=np.zeros(s["n"], np.uint8))


def _oracle_step(s, t, act_a, act_b, **uniforms):
    o = s["o"]
    _inject(o, s, t); o.tick = TICK0
    return o.step(act_a, act_b, **uniforms)


@pytest.mark.parametrize("name,slip,entry", [(name, slip, entry) for name in NAMES for slip in SLIPS for entry in ("philox", "policy", "uniforms")])
def test_one_step_from_every_tuple_and_action_pair(name, slip, entry):
    """philox: the handle's own draws, at t = max_steps - 1 (a step that does not score truncates) and at t = 0, lean and full
    outputs, and at t = max_steps - 1 also through buffers that start one element into their allocations (the whole step is byte
    I/O on the per-lane kernel).  policy: one player by policy[observation] (B at slip 0, A at slip 0.2).  uniforms: caller-supplied
    u_step / u_reset.  The last two at t = max_steps - 1.  The lane count is 3 modulo 4: every step has a ragged tail of three."""
    c = CASES[name]
    s = _sweep(name, slip)
    n, aa, ab = s["n"], s["aa"], s["ab"]
    rng = np.random.default_rng(NAMES.index(name) * 10 + int(slip * 10))
    b = SoccerBatch(n, c["w"], c["h"], slip, seed=SEED, autoreset=True, max_steps=MAX_STEPS, step_stats=False)
    assert b.nS == c["nS"] and b.state_streams() == (3 if c["packs"] else 6) and b.n_isd == c["kickoffs"]
    r = _reached(name)
    r["streams"].add(b.state_streams()); r["lut_lds"].add(c["lut_lds"])
    seen = None
    if entry == "philox":
        ios = (_IO(b, True), _IO(b, False))
        for t in (MAX_STEPS - 1, 0):
            exp = _oracle_step(s, t, aa, ab)
            seen = seen or lp.reach_of_step(c, s["st"], exp)
            for io in ios:
                _inject(b, s, t); _set_tick(b, TICK0)
                _check(io.step(aa, ab), exp, t)
                _state_equal(b, s["o"])
            if t == 0:
                assert c["nS"] <= 32768 or exp["obs"].max() >= 32768          # nothing truncates: obs is the tuple stepped to
                assert not exp["truncated"].any()
                continue
            sh = _ShiftedIO(b, shift=1)
            _inject(b, s, t); _set_tick(b, TICK0)
            got = sh.step(aa, ab, True, None, None)
            for key in ("obs", "reward", "terminated", "truncated", "prob_code", "final_obs"):
                np.testing.assert_array_equal(got[key], exp[key], err_msg="%s through shifted buffers" % key)
            np.testing.assert_array_equal(got["done"], exp["terminated"] | exp["truncated"])
            np.testing.assert_array_equal(got["rfa"], exp["reward"].astype(np.float32))
            _state_equal(b, s["o"])
    elif entry == "policy":
        fixed = "player_b" if slip == 0.0 else "player_a"
        policy = _fixed_policy(rng, c["nS"])
        assert s["cur"].max() == c["nS"] - 1 and (s["cur"] == 0).sum() >= 25          # the goal tuples look up policy[0]
        ea, eb = (policy[s["cur"]], ab) if fixed == "player_a" else (aa, policy[s["cur"]])
        exp = _oracle_step(s, MAX_STEPS - 1, ea, eb)
        seen = lp.reach_of_step(c, s["st"], exp)
        b.set_policy(fixed, policy)
        for io in (_IO(b, True), _IO(b, False)):
            _inject(b, s, MAX_STEPS - 1); _set_tick(b, TICK0)
            _check(io.step(None if fixed == "player_a" else aa, None if fixed == "player_b" else ab), exp, MAX_STEPS - 1)
            _state_equal(b, s["o"])
    else:
        us, ur = rng.random(n), rng.random(n)
        exp = _oracle_step(s, MAX_STEPS - 1, aa, ab, u_step=us, u_reset=ur)
        seen = lp.reach_of_step(c, s["st"], exp)
        U = b.alloc(n, np.float64).upload(us); UR = b.alloc(n, np.float64).upload(ur)
        for full in (True, False):
            io = _IO(b, full)
            _inject(b, s, MAX_STEPS - 1); _set_tick(b, TICK0)
            io.aa.upload(aa); io.ab.upload(ab)
            b.step(io.aa, io.ab, obs=io.obs, reward=io.rew, terminated=io.term, truncated=io.trunc, prob_code=io.code, final_obs=io.fin,
                   u_step=U, u_reset=UR)
            got = dict(obs=io.obs.download(), reward=io.rew.download(), terminated=io.term.download(), truncated=io.trunc.download())
            if full:
                got.update(prob_code=io.code.download(), final_obs=io.fin.download())
            _check(got, exp, MAX_STEPS - 1)
            _state_equal(b, s["o"])
    # the oracle's side reached what the case is for (also shown without a GPU), and nothing was flagged on the device
    floors = lp.sweep_floors(c)
    assert (seen["row"], seen["col"]) == (c["H"] - 1, c["W"] - 1) and (c["nS"] <= 32768 or seen["final_obs"] >= 32768)
    assert seen["plus"] >= floors["plus"] and seen["minus"] >= floors["minus"] and seen["truncated"] >= floors["truncated"]
    assert b.misuse() == 0 and b.tick == TICK0 + 1
    b.close()


# ---- (b) rollouts ----------------------------------------------------------------------------------------------------------------
_TABLES = {}


def _tables(name):
    """the observation-keyed inputs of a case's rollouts: two mixed-policy threshold tables and a fixed policy, made once"""
    if name not in _TABLES:
        _TABLES.clear()
        rng = np.random.default_rng(500 + NAMES.index(name))
        nS = CASES[name]["nS"]
        _TABLES[name] = dict(mix=(_threshold_rows(rng, nS), _threshold_rows(rng, nS)), policy=_fixed_policy(rng, nS))
    return _TABLES[name]


ROLLOUT_SOURCES = ("streams", "uniform", "both_mixed", "fixed_a_stream_b")


def _check_rollout_shape(sh, c, slip, source, extras):
    tables = source in ("both_mixed", "fixed_a_stream_b")
    assert sh["small_pitch"] == int(c["small"]) and sh["full"] == int(extras) and sh["chunks"] == 1
    if not c["fits"]:
        assert (sh["kernel"], sh["tail"], sh["parts"], sh["slip_selection"]) == (PER_LANE, 0, 1, int(slip != 0.0))
        assert sh["dynamic_lds_bytes"] == c["lds_bytes"] <= sh["lds_limit"]
        assert sh["table_placement"] == (GLOBAL if tables else NONE)
    elif source == "streams":
        assert (sh["kernel"], sh["tail"], sh["parts"], sh["action_source"], sh["table_placement"]) == (BYTE_PARALLEL, 1, 1, 0, NONE)
        assert sh["dynamic_lds_bytes"] == ((SLIP_ROWS_BYTES + 15) & ~15) + STAGING_BYTES
    else:
        _check_shape(sh, c["nS"], N, T, source, BYTE_PARALLEL, 0 if slip == 0.0 else 2, extras)


@pytest.mark.parametrize("name,slip", [(name, slip) for name in NAMES for slip in SLIPS])
def test_rollouts_of_every_action_source(name, slip):
    """T = 48 steps on 4096 + 3 lanes, rows 4096 + 4 apart, from lp.rollout_start: streamed actions, uniform sampling, both players
    mixed, a fixed policy against a stream, each with and without the per-step final_obs / prob_code.  Handles beyond the byte
    arithmetic run every source at 1, 4 and 8 lanes per thread (rows 4096 + 8 apart for 8: with rows a multiple of 4 apart the
    launch would take 4), which launches rollout_kernel<1|4|8, slip, lut_lds, false|true> of the handle's placement; the others
    run the per-lane kernel on their last three lanes."""
    c = CASES[name]
    tab = _tables(name)
    o = Oracle(c["w"], c["h"], slip, n=N, seed=SEED, autoreset=True, max_steps=MAX_STEPS)
    r = _reached(name)
    run = 0
    for epw in ((0,) if c["fits"] else (1, 4, 8)):
        for source in ROLLOUT_SOURCES:
            for extras in ((False, True) if c["fits"] else (bool((run + epw) & 1),)):
                run += 1
                rng = np.random.default_rng(run)
                o.tick = 0; o.hist[:] = 0; o.misuse = 0
                b = SoccerBatch(N, c["w"], c["h"], slip, seed=SEED, autoreset=True, max_steps=MAX_STEPS, envs_per_thread=epw)
                assert b.state_streams() == (3 if c["packs"] else 6)
                b.reset(); o.reset()
                st = lp.rollout_start(o, rng)
                b.set_state(**st); o.set_state(**st)
                sample, use_a, use_b, fixed = SOURCES[source] if source != "streams" else (False, False, False, None)
                acts = None if sample else rng.integers(0, 5, size=(T, 2, N), dtype=np.int8)
                if fixed:
                    b.set_policy(fixed, tab["policy"])

                def floors(seen):
                    for k in ("plus", "minus"):
                        assert seen[k] >= lp.ROLLOUT_FLOORS[k], (k, seen[k])
                    assert int(seen["episodes"].sum()) - seen["plus"] - seen["minus"] >= lp.ROLLOUT_FLOORS["truncated"]
                _rollout_vs_oracle(b, o, acts, T, N, sample=sample, mix=tab["mix"] if use_a else None, extras=extras,
                                   policy=tab["policy"] if fixed else None, fixed=fixed, precheck=floors, strict=True,
                                   stride=STRIDE + 4 if epw == 8 else STRIDE)
                sh = b.rollout_shape()
                _check_rollout_shape(sh, c, slip, source, extras)
                r["kernels"].add(sh["kernel"]); r["streams"].add(b.state_streams()); r["small"].add(sh["small_pitch"])
                r["lut_lds"].add(c["lut_lds"])
                if sh["kernel"] == PER_LANE:
                    r["per_lane_lds"].add(sh["dynamic_lds_bytes"])
                b.close()
    print("%-6s slip %.1f: %d rollouts, the last one %s" % (name, slip, run, sh))


# ---- (c) resets ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_resets_full_masked_and_with_caller_uniforms(name):
    """on 4096 + 3 lanes: the byte-parallel reset takes the first 4096 where the pitch fits it and the per-lane kernel the last three;
    with caller uniforms, and on every other pitch, reset_kernel<lut_lds, slip> takes them all — with 152 064 B of LDS on 36x5"""
    c = CASES[name]
    for slip in SLIPS:
        rng = np.random.default_rng(NAMES.index(name))
        b = SoccerBatch(N, c["w"], c["h"], slip, seed=SEED, autoreset=False, max_steps=MAX_STEPS)
        o = Oracle(c["w"], c["h"], slip, n=N, seed=SEED, autoreset=False, max_steps=MAX_STEPS)
        obs = b.alloc(N, np.uint16).fill(0xEE); mask = b.alloc(N, np.uint8); U = b.alloc(N, np.float64)
        b.reset(obs=obs)
        want = o.reset()
        np.testing.assert_array_equal(obs.download(), want, err_msg="full reset")
        assert len(np.unique(want)) == c["kickoffs"] and (want > 0).all()
        _state_equal(b, o)
        st = lp.rollout_start(o, rng)
        st["needs_reset"] = (rng.random(N) < 0.3).astype(np.uint8)
        b.set_state(**st); o.set_state(**st)
        m = np.array([0, 1, 255, 128, 0, 0, 2, 0], np.uint8)[rng.integers(0, 8, size=N)]
        b.reset(mask=mask.upload(m), obs=obs)
        want = o.reset(mask=m)
        np.testing.assert_array_equal(obs.download(), want, err_msg="masked reset")       # the lanes left alone report the tuple they hold
        assert c["nS"] <= 32768 or want.max() >= 32768
        _state_equal(b, o)
        edges = np.array([0.0, 0.25, 0.5, 0.75, np.nextafter(0.25, 0), np.nextafter(0.5, 0), np.nextafter(0.75, 0), 1.0 - 2.0 ** -53])
        u = np.where(rng.random(N) < 0.25, edges[rng.integers(0, len(edges), N)], rng.random(N))
        b.reset(u_reset=U.upload(u), obs=obs)
        want = o.reset(u_reset=u)
        np.testing.assert_array_equal(obs.download(), want, err_msg="reset with caller uniforms")
        assert len(np.unique(want)) == c["kickoffs"]
        _state_equal(b, o)
        b.reset(mask=mask.upload(m), u_reset=U, obs=obs)
        np.testing.assert_array_equal(obs.download(), o.reset(mask=m, u_reset=u), err_msg="masked reset with caller uniforms")
        _state_equal(b, o)
        assert b.tick == o.tick == 4 and b.misuse() == 0
        # what the per-lane kernels of this handle are launched with: a one-step rollout that has to take the per-lane kernel (a
        # reward stream no vector store can write) reports it
        rew = b.alloc(N + 8, np.int8)
        b.rollout(1, sample_actions=True, reward=rew.ptr + 1, out_stride=N + 4)
        sh = b.rollout_shape()
        assert sh["kernel"] == PER_LANE and sh["dynamic_lds_bytes"] == c["lds_bytes"] <= sh["lds_limit"]
        _reached(name)["per_lane_lds"].add(sh["dynamic_lds_bytes"])
        b.close()
    print("%-6s per-lane dynamic_lds_bytes %d (observation table %s)" % (name, sh["dynamic_lds_bytes"], "in LDS" if c["lut_lds"] else "in global memory"))


# ---- (d) acceptance and refusal ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lp.ACCEPTED_AT_THE_LIMIT)
def test_the_largest_pitches_are_accepted(name):
    c = CASES[name]
    n = 259
    b = SoccerBatch(n, c["w"], c["h"], 0.2, seed=SEED, autoreset=True, max_steps=MAX_STEPS)
    assert b.nS == lp.LARGEST_NS == 64441 and b.internal_width == c["W"] and b.n_isd == c["kickoffs"] and b.lut_len == c["lut_bytes"] // 2
    obs = b.alloc(n, np.uint16); rew = b.alloc(n, np.int8); A = b.alloc(n, np.int8).fill(3); B = b.alloc(n, np.int8).fill(4)
    b.reset(obs=obs)
    assert (obs.download() > 0).all()
    for _ in range(3):
        b.step(A, B, obs=obs, reward=rew)
    got = obs.download()
    assert (got > 0).all() and (got < b.nS).all() and b.tick == 4 and b.misuse() == 0
    b.close()
    assert b.h is None


@pytest.mark.parametrize("wh,text", lp.REFUSED, ids=["%dx%d" % wh for wh, _ in lp.REFUSED])
def test_pitches_beyond_the_limits_are_refused_with_the_library_s_text(wh, text):
    w, h = wh
    assert text in lp.refusal(w, h)
    with pytest.raises(AssertionError) as e:
        SoccerBatch(64, w, h, 0.0, seed=1)
    assert text in str(e.value)
    if w < 5 or h < 4:
        assert str(e.value) == text                              # the reference's own wording, whole
    # straight through soccer_create: the code, the text, and no handle left behind
    lib = _lib.load()
    cfg = _lib.Config(n_lanes=64, width=w, height=h, slip_prob=0.0, max_steps=100, device=0, seed=1, lane_offset=0, flags=0,
                      envs_per_thread=0, stream=None)
    out = C.c_void_p(0xDEAD)
    assert lib.soccer_create(C.byref(cfg), C.byref(out)) == _lib.E_INVALID
    assert out.value is None and text in lib.soccer_last_error(None).decode()


def test_zz_the_cases_reached_every_placement():
    """what tests (a) - (c) of this module saw, case by case: both kernels, both layouts, both geometries, the observation table in
    LDS and in global memory, and a per-lane launch with more than 150 000 B of dynamic LDS"""
    assert sorted(_REACHED) == sorted(NAMES), "run the whole module"
    for name in NAMES:
        c, r = CASES[name], _REACHED[name]
        print("%-6s kernels %s streams %s small %s lut_lds %s per-lane LDS %s" % (name, sorted(r["kernels"]), sorted(r["streams"]), sorted(r["small"]),
                                                                                  sorted(r["lut_lds"]), sorted(r["per_lane_lds"])))
        assert r["kernels"] == ({BYTE_PARALLEL} if c["fits"] else {PER_LANE}) and r["streams"] == {3 if c["packs"] else 6}
        assert r["small"] == {int(c["small"])} and r["lut_lds"] == {c["lut_lds"]} and r["per_lane_lds"] == {c["lds_bytes"]}
    every = lambda k: set().union(*(_REACHED[name][k] for name in NAMES))
    assert every("kernels") == {BYTE_PARALLEL, PER_LANE} and every("streams") == {3, 6} and every("small") == {0, 1}
    assert every("lut_lds") == {False, True} and max(every("per_lane_lds")) == lp.LARGEST_LDS > 150000
    # byte-parallel kernels on six streams that are the handle's by nature
    assert {name for name in NAMES if CASES[name]["fits"] and not CASES[name]["packs"]} == {"15x4", "30x4", "5x9", "5x18"}
