"""How step_kernel_swar gets its arguments: the leading scalars arrive preloaded (the action-load policy in bit 0 of the lane
count), everything else is one struct whose layout every shape of the kernel has to read correctly, and the step is evaluated
in two parts (swar::step4_moves ahead of the state, swar::step4_state behind it).  None of that may change a bit: every case
drives a small handle — n = 260: one full wave plus a wave with a single active thread, lane_offset 8, auto-reset after 5
steps so that resets happen — for 12 steps and compares EVERY output stream and get_state lane for lane with the oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gym_soccer_littman94_amd import SoccerBatch
from oracle.oracle import Oracle

N, STEPS, MAX_STEPS, OFFSET = 260, 12, 5, 8
PLAIN = ("obs", "reward", "terminated", "truncated")


def _state_equal(b, o, what=""):
    s = b.get_state()
    for k, v in (("row_a", o.row_a), ("col_a", o.col_a), ("row_b", o.row_b), ("col_b", o.col_b), ("poss", o.poss & 1),
                 ("needs_reset", (o.poss >> 1) & 1), ("t", o.t)):
        np.testing.assert_array_equal(s[k], v, err_msg="%s %s" % (k, what))


def _make(monkeypatch, n=N, w=5, h=4, slip=0.0, wide=False, autoreset=True, seed=3, **kw):
    if wide: monkeypatch.setenv("SOCCER_STATE_LAYOUT", "wide")
    b = SoccerBatch(n, w, h, slip, seed=seed, autoreset=autoreset, max_steps=MAX_STEPS, lane_offset=OFFSET, **kw)
    if wide: monkeypatch.delenv("SOCCER_STATE_LAYOUT")
    assert b.state_streams() == (6 if wide else 3)
    return b


def _oracle(n=N, w=5, h=4, slip=0.0, autoreset=True, seed=3):
    return Oracle(w, h, slip, n=n, seed=seed, autoreset=autoreset, lane_offset=OFFSET, max_steps=MAX_STEPS)


class _IO:
    """the device buffers of one handle; step() returns every stream that was asked for"""
    NAMES = dict(obs=np.uint16, reward=np.int8, terminated=np.uint8, truncated=np.uint8, prob_code=np.uint8, final_obs=np.uint16,
                 reward_a_f32=np.float32, reward_b_f32=np.float32, finished=np.uint8, last_return=np.int8)

    def __init__(self, b):
        self.b = b
        self.aa, self.ab = b.alloc(b.n, np.int8), b.alloc(b.n, np.int8)
        self.us, self.ur = b.alloc(b.n, np.float64), b.alloc(b.n, np.float64)
        self.first = b.alloc(b.n, np.uint16)                   # the observation of a reset
        self.out = {k: b.alloc(b.n, dt) for k, dt in self.NAMES.items()}
        for a in self.out.values(): a.fill(0x55)

    def step(self, a0, a1, want=PLAIN, u_step=None, u_reset=None):
        if a0 is not None: self.aa.upload(a0)
        if a1 is not None: self.ab.upload(a1)
        if u_step is not None: self.us.upload(u_step)
        if u_reset is not None: self.ur.upload(u_reset)
        self.b.step(self.aa if a0 is not None else None, self.ab if a1 is not None else None,
                    u_step=self.us if u_step is not None else None, u_reset=self.ur if u_reset is not None else None,
                    **{k: self.out[k] for k in want})
        return {k: self.out[k].download() for k in want}


def _acts(rng, n=N):
    return rng.integers(0, 5, size=(2, n), dtype=np.int8)


def _check(got, c, keys, what):
    for key in keys:
        np.testing.assert_array_equal(got[key], c[key], err_msg="%s %s" % (key, what))


def _drive(b, o, rng, want=PLAIN, steps=STEPS, uniforms=False):
    """reset, then `steps` steps of random actions: the streams in `want` that the oracle knows, the tick and the final state"""
    io = _IO(b)
    b.reset(obs=io.first)
    np.testing.assert_array_equal(io.first.download(), o.reset())
    resets = 0
    for k in range(steps):
        a = _acts(rng, b.n)
        us, ur = (rng.random(b.n), rng.random(b.n) if k % 3 else None) if uniforms else (None, None)
        c = o.step(a[0], a[1], u_step=us, u_reset=ur)
        got = io.step(a[0], a[1], want, us, ur)
        _check(got, c, [key for key in want if key in c], "at step %d" % k)
        assert b.tick == o.tick
        resets += int((c["terminated"] | c["truncated"]).sum())
    assert resets > 0                                          # the auto-reset was exercised
    _state_equal(b, o)
    return io


@pytest.mark.parametrize("layout", ["packed", "wide"])
@pytest.mark.parametrize("w,h", [(5, 4), (7, 5)])              # byte-table geometry (GEO = 1) / arithmetic geometry (GEO = 0)
@pytest.mark.parametrize("slip", [0.0, 0.2, 0.03])             # no slip / selection by table / one-by-one selection
def test_both_action_load_policies_give_the_oracles_bytes(monkeypatch, slip, w, h, layout):
    rng = np.random.default_rng(5)
    o = _oracle(w=w, h=h, slip=slip)
    pair = [_make(monkeypatch, w=w, h=h, slip=slip, wide=layout == "wide", stream_actions=sa, step_stats=False) for sa in (True, False)]
    ios = [_IO(b) for b in pair]
    exp = o.reset()
    for b, io in zip(pair, ios):
        b.reset(obs=io.first)
        np.testing.assert_array_equal(io.first.download(), exp)
    for k in range(STEPS):
        a = _acts(rng)
        c = o.step(a[0], a[1])
        got = [io.step(a[0], a[1]) for io in ios]
        for g, sa in zip(got, (True, False)):
            _check(g, c, PLAIN, "at step %d (stream_actions=%s)" % (k, sa))
        _check(got[0], got[1], PLAIN, "at step %d: the two policies differ" % k)
    for b in pair:
        _state_equal(b, o)
        assert b.stats()[1] == 0 and b.tick == o.tick
        b.close()


@pytest.mark.parametrize("slip", [0.0, 0.2])
def test_a_launch_part_size_that_is_no_multiple_of_4_is_rounded_down(monkeypatch, slip):
    """514 -> 512 lanes per launch: parts of 512, 512 and 12 lanes, each with a lane count whose low bits are free for the policy;
    same results, and the tick advances once per step (only the last part publishes it)"""
    n = 1036
    monkeypatch.setenv("SOCCER_SWAR_LAUNCH_LANES", "514")
    pair = [_make(monkeypatch, n=n, slip=slip, stream_actions=sa, step_stats=False) for sa in (True, False)]
    monkeypatch.delenv("SOCCER_SWAR_LAUNCH_LANES")
    for b in pair:
        o = _oracle(n=n, slip=slip)
        _drive(b, o, np.random.default_rng(7))
        assert b.tick == o.tick and b.stats()[1] == 0
        b.close()


@pytest.mark.parametrize("missing", PLAIN)
def test_each_result_stream_may_be_null(monkeypatch, missing):
    b, o = _make(monkeypatch, step_stats=False), _oracle()
    want = tuple(k for k in PLAIN if k != missing)
    io = _drive(b, o, np.random.default_rng(11), want=want)
    assert (io.out[missing].download().view(np.uint8) == 0x55).all()      # and nothing was written through a stale pointer
    b.close()


@pytest.mark.parametrize("slip", [0.0, 0.2])
@pytest.mark.parametrize("shape", ["gym_outputs", "info"])
def test_the_info_shapes(monkeypatch, shape, slip):
    """OUT = 1: + the float rewards / finished / last_return; OUT = 2: + prob_code / final_obs and the episode histogram"""
    full = shape == "info"
    b, o = _make(monkeypatch, slip=slip, step_stats=full), _oracle(slip=slip)
    want = PLAIN + ("reward_a_f32", "reward_b_f32", "finished", "last_return") + (("prob_code", "final_obs") if full else ())
    io = _IO(b)
    b.reset()
    o.reset()
    rng = np.random.default_rng(13)
    last = np.full(N, 0x55, np.int8)
    for k in range(STEPS):
        a = _acts(rng)
        c = o.step(a[0], a[1])
        got = io.step(a[0], a[1], want)
        _check(got, c, PLAIN + (("prob_code", "final_obs") if full else ()), "at step %d" % k)
        r = c["reward"].astype(np.float32)
        np.testing.assert_array_equal(got["reward_a_f32"].view(np.uint32), r.view(np.uint32))
        np.testing.assert_array_equal(got["reward_b_f32"].view(np.uint32), (np.float32(0) - r).view(np.uint32))
        done = c["terminated"] | c["truncated"]
        np.testing.assert_array_equal(got["finished"], done)
        last = np.where(done != 0, c["reward"], last)
        np.testing.assert_array_equal(got["last_return"], last)
    hist, misuse = b.stats()
    assert misuse == 0 and b.tick == o.tick
    if full:
        np.testing.assert_array_equal(hist, o.hist)
        assert o.hist.sum() > 0
    _state_equal(b, o)
    b.close()


@pytest.mark.parametrize("fixed", ["player_a", "player_b"])
def test_a_single_agent_handle(monkeypatch, fixed):
    b, o = _make(monkeypatch, step_stats=False), _oracle()
    rng = np.random.default_rng(17)
    policy = rng.integers(0, 5, size=o.nS).astype(np.int8)
    b.set_policy(fixed, policy)
    io = _IO(b)
    b.reset(obs=io.first)
    cur = o.reset()
    np.testing.assert_array_equal(io.first.download(), cur)
    for k in range(STEPS):
        act = rng.integers(0, 5, size=N, dtype=np.int8)
        c = o.step(*((policy[cur], act) if fixed == "player_a" else (act, policy[cur])))
        got = io.step(None if fixed == "player_a" else act, None if fixed == "player_b" else act)
        _check(got, c, PLAIN, "at step %d" % k)
        cur = c["obs"]
    _state_equal(b, o)
    assert b.stats()[1] == 0 and b.tick == o.tick
    b.close()


@pytest.mark.parametrize("slip", [0.0, 0.2])                   # EXPL / SLIPM == 3 (with its work list)
def test_caller_supplied_uniforms(monkeypatch, slip):
    b, o = _make(monkeypatch, slip=slip, step_stats=False), _oracle(slip=slip)
    _drive(b, o, np.random.default_rng(19), uniforms=True)
    assert b.stats()[1] == 0
    b.close()


@pytest.mark.parametrize("slip", [0.0, 0.2])
def test_a_captured_graph_reads_the_tick_from_the_device_slot(monkeypatch, slip):
    """9 steps captured, replayed twice, against 18 eager steps of the oracle"""
    T = 9
    b, o = _make(monkeypatch, slip=slip, step_stats=False), _oracle(slip=slip)
    rng = np.random.default_rng(23)
    b.reset()
    o.reset()
    acts = rng.integers(0, 5, size=(T, 2, N), dtype=np.int8)
    A = b.alloc((T, N), np.int8).upload(acts[:, 0]); B = b.alloc((T, N), np.int8).upload(acts[:, 1])
    O = b.alloc((T, N), np.uint16); R = b.alloc((T, N), np.int8); TE = b.alloc((T, N), np.uint8); TR = b.alloc((T, N), np.uint8)
    b.graph_begin()
    for k in range(T):
        b.step_plain(A.row(k), B.row(k), O.row(k), R.row(k), TE.row(k), TR.row(k))
    g = b.graph_end()
    for rep in range(2):
        b.graph_launch(g, 1)
        got = dict(obs=O.download(), reward=R.download(), terminated=TE.download(), truncated=TR.download())
        for k in range(T):
            c = o.step(acts[k, 0], acts[k, 1])
            _check({key: v[k] for key, v in got.items()}, c, PLAIN, "at step %d of replay %d" % (k, rep))
        assert b.tick == o.tick
    b.graph_destroy(g)
    _state_equal(b, o)
    b.close()


@pytest.mark.parametrize("slip", [0.0, 0.2])
def test_one_action_byte_of_7_is_reported_and_executes_as_noop(monkeypatch, slip):
    b, o = _make(monkeypatch, slip=slip, step_stats=False), _oracle(slip=slip)
    rng = np.random.default_rng(29)
    io = _IO(b)
    b.reset()
    o.reset()
    for k in range(STEPS):
        a = _acts(rng)
        sent = a.copy()
        if k == 4:
            a[1, 257] = 0; sent[1, 257] = 7                    # the lone thread of the second wave
            assert b.stats()[1] == 0
        c = o.step(a[0], a[1])
        _check(io.step(sent[0], sent[1]), c, PLAIN, "at step %d" % k)
        if k >= 4: assert b.peek_misuse() == SoccerBatch.MISUSE_ACTION
    _state_equal(b, o)
    assert b.stats()[1] == SoccerBatch.MISUSE_ACTION
    b.close()


@pytest.mark.parametrize("layout", ["packed", "wide"])
def test_goal_tuples_injected_into_a_handle_without_autoreset(monkeypatch, layout):
    """no auto-reset: every thread takes the GENERAL step, which derives the move tables again from the held actions"""
    b = _make(monkeypatch, wide=layout == "wide", autoreset=False, step_stats=False)
    o = _oracle(autoreset=False)
    rng = np.random.default_rng(31)
    io = _IO(b)
    b.reset()
    o.reset()
    lut, kind, *_ = o.tables()
    f = np.concatenate([np.flatnonzero(kind == 1), np.flatnonzero(kind == 2), np.flatnonzero(kind == 2)])
    f = f[rng.integers(0, len(f), size=N)]
    assert (kind[f] == 2).sum() > 20
    poss = f & 1; r = f >> 1
    cb = r % o.W; r //= o.W; rb = r % o.H; r //= o.H; ca = r % o.W; ra = r // o.W
    t = np.zeros(N, np.uint8); need = np.zeros(N, np.uint8)
    o.set_state(ra, ca, rb, cb, poss, t=t, needs_reset=need)
    b.set_state(ra, ca, rb, cb, poss, t=t, needs_reset=need)
    for k in range(STEPS):                                     # the lanes freeze at step 5; stepping them on is the reported misuse
        a = _acts(rng)
        c = o.step(a[0], a[1])
        _check(io.step(a[0], a[1], PLAIN + ("prob_code", "final_obs") if k & 1 else PLAIN), c,
               PLAIN + (("prob_code", "final_obs") if k & 1 else ()), "at step %d" % k)
    _state_equal(b, o)
    assert b.stats()[1] == SoccerBatch.MISUSE_FROZEN and b.tick == o.tick
    b.close()
