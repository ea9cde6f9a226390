"""-m gpu: what every entry point of the six kinds of learners refuses before it touches anything, with the exact text (the
texts are those of the sources before the kinds shared their host code: one check per kind then, one for all now), and the
lifetime of learners of different kinds on one handle.  A 5x4 pitch without slip, 64 lanes.

The entry points of a kind come from one table; an entry point's arguments behind (handle, learner) are zeros and NULLs:
every refusal here precedes their first use."""
import ctypes as C
import re

import numpy as np
import pytest

from gym_soccer_littman94_amd import SoccerBatch, _lib

pytestmark = pytest.mark.gpu

GAMMA, N = 0.9, 64
SINGLE = ("destroy", "run", "update", "read", "load")
# kind: (constructor, the prefix of its C entry points, what a message calls it, its entry points that take a learner)
KINDS = {
    "minimax_q": (lambda b: b.minimax_q(GAMMA), "soccer_minimax_q", "learner", SINGLE),
    "q_learner": (lambda b: b.q_learning(GAMMA), "soccer_q_learner", "learner", SINGLE),
    "wolf_phc": (lambda b: b.wolf_phc(GAMMA), "soccer_wolf_phc", "learner", SINGLE),
    "q_population": (lambda b: b.q_population(GAMMA), "soccer_q_population", "population", SINGLE + ("league_read", "league_load")),
    "wolf_population": (lambda b: b.wolf_population(GAMMA), "soccer_wolf_population", "population", SINGLE + ("adopt",)),
    "minimax_q_population": (lambda b: b.minimax_q_population(GAMMA), "soccer_minimax_q_population", "population", SINGLE),
}
CREATES = {k: ("create",) for k in KINDS}
CREATES["q_population"] = ("create", "create_league")


def said(prefix, entry):
    """the name an entry point gives itself in a message"""
    return prefix + "_" + entry + (" (dst)" if entry == "adopt" else "")


def call(b, name, h, *given):
    """the C function `name` on handle h: `given` fills its leading arguments behind the handle (a learner, then the integers
    in their order), zeros and NULLs the rest"""
    types = _lib.PROTOTYPES[name][1][1:]
    args = list(given) + [0 if t in (C.c_int32, C.c_int64) else None for t in types[len(given):]]
    return getattr(b.lib, name)(h, *args)


def refused(exc, text):
    return pytest.raises(exc, match="^" + re.escape(text) + "$")


def batch(**kw):
    return SoccerBatch(N, 5, 4, 0.0, seed=7, **{"autoreset": True, **kw})


@pytest.fixture(scope="module")
def six():
    """one handle with a live learner of every kind"""
    b = batch()
    yield b, {k: KINDS[k][0](b) for k in KINDS}
    b.close()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_null_handle(six, kind):
    b, live = six
    _, prefix, _, entries = KINDS[kind]
    for entry in entries:
        with refused(AssertionError, "handle is NULL"):
            _lib.check(b.lib, None, call(b, prefix + "_" + entry, None, live[kind].q))
    for entry in CREATES[kind]:
        with refused(AssertionError, "handle is NULL"):
            _lib.check(b.lib, None, call(b, prefix + "_" + entry, None))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_call_during_graph_capture(six, kind):
    b, live = six
    _, prefix, _, entries = KINDS[kind]
    b.sync()
    b.graph_begin()
    try:
        b.rollout(2, sample_actions=True)           # (something to capture; never replayed)
        for entry in entries:
            with refused(RuntimeError, said(prefix, entry) + " during graph capture"):
                b._check(call(b, prefix + "_" + entry, b.h, live[kind].q))
        for entry in CREATES[kind]:
            with refused(RuntimeError, prefix + "_" + entry + " during graph capture"):
                b._check(call(b, prefix + "_" + entry, b.h))
    finally:
        b.graph_destroy(b.graph_end())
    assert live[kind].run(1).steps >= 1             # nothing was destroyed


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_learner_of_another_handle(six, kind):
    b, live = six
    _, prefix, noun, entries = KINDS[kind]
    other = batch()
    try:
        for entry in entries:
            with refused(AssertionError, "%s: not a %s of this handle" % (said(prefix, entry), noun)):
                other._check(call(other, prefix + "_" + entry, other.h, live[kind].q))
    finally:
        other.close()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_destroyed_learner(kind):
    """the check compares addresses and never reads through the pointer; nothing is created in between"""
    ctor, prefix, noun, entries = KINDS[kind]
    b = batch()
    try:
        q = ctor(b)
        gone = C.c_void_p(q.q.value)
        q.close()
        for entry in entries:
            with refused(AssertionError, "%s: not a %s of this handle" % (said(prefix, entry), noun)):
                b._check(call(b, prefix + "_" + entry, b.h, gone))
    finally:
        b.close()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_learner_of_each_other_kind(six, kind):
    b, live = six
    _, prefix, noun, entries = KINDS[kind]
    for other in sorted(KINDS):
        if other == kind:
            continue
        raw = C.c_void_p(live[other].q.value)
        for entry in entries:
            with refused(AssertionError, "%s: not a %s of this handle" % (said(prefix, entry), noun)):
                b._check(call(b, prefix + "_" + entry, b.h, raw))
    if kind == "wolf_population":                    # ... and as the second population of an adopt
        for other in sorted(KINDS):
            if other != kind:
                with refused(AssertionError, "soccer_wolf_population_adopt (src): not a population of this handle"):
                    b._check(b.lib.soccer_wolf_population_adopt(b.h, live[kind].q, 0, C.c_void_p(live[other].q.value), 0, 0))
    for q in live.values():                          # every one of them is still what it was
        assert q.run(1).steps >= 1


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_negative_number_of_steps(six, kind):
    b, live = six
    prefix = KINDS[kind][1]
    for n_steps in (-1, -2 ** 31):
        with refused(AssertionError, prefix + "_run: n_steps must be >= 0"):
            b._check(call(b, prefix + "_run", b.h, live[kind].q, n_steps))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_handle_without_autoreset_and_a_handle_with_a_fixed_policy(kind):
    ctor, prefix = KINDS[kind][:2]
    plain = batch(autoreset=False)
    try:
        with refused(AssertionError, prefix + "_create needs a handle created with SOCCER_F_AUTORESET"):
            ctor(plain)
        plain.set_policy(1, np.zeros(plain.nS, np.int8))      # (the fixed policy is what is named when both are wrong)
        with refused(AssertionError, prefix + "_create needs a two-player handle: neither side may have a fixed policy (soccer_set_policy)"):
            ctor(plain)
    finally:
        plain.close()
    for player in (0, 1):
        single = batch()
        try:
            single.set_policy(player, np.zeros(single.nS, np.int8))
            with refused(AssertionError, prefix + "_create needs a two-player handle: neither side may have a fixed policy (soccer_set_policy)"):
                ctor(single)
        finally:
            single.close()


@pytest.mark.parametrize("kind", [k for k in sorted(KINDS) if KINDS[k][2] == "population"])
def test_members_outside_the_population(six, kind):
    b, live = six
    prefix = KINDS[kind][1]
    for first, count in ((-1, 1), (0, -1), (0, N + 1), (N + 1, 0), (1, N), (N, 1), (2 ** 62, 2 ** 62)):
        for entry in ("read", "load"):
            with refused(AssertionError, "%s_%s: members %d .. %d + %d are outside the population of %d" % (prefix, entry, first, first, count, N)):
                b._check(call(b, prefix + "_" + entry, b.h, live[kind].q, first, count))
    for first, count in ((0, N), (N, 0), (N - 1, 1), (0, 0)):      # the edges inside
        assert live[kind].read(first, count)["alpha"].shape == (count,)


# ---- lifetime ------------------------------------------------------------------------------------
def test_destroying_out_of_creation_order_leaves_the_rest_usable():
    b = batch()
    try:
        b.reset()                                    # (a lane is frozen until its first reset)
        order = ("q_population", "minimax_q", "wolf_population", "q_learner", "minimax_q_population", "wolf_phc")
        live = {k: KINDS[k][0](b) for k in order}
        for k in ("minimax_q_population", "q_population", "q_learner"):     # the fifth, the first, the fourth: three kinds
            live.pop(k).close()
        for k, q in live.items():
            assert q.run(3).steps == 3, k
        again = KINDS["q_population"][0](b)          # a new one after the gaps, and the old ones after it
        assert again.run(2).steps == 2
        for k, q in live.items():
            assert q.run(1).steps == 4, k
        again.close()
        for q in live.values():
            q.close()
        assert b.misuse() == 0
    finally:
        b.close()


def test_a_handle_closed_with_learners_of_all_six_kinds_alive_frees_them():
    b = batch()
    b.reset()
    live = [KINDS[k][0](b) for k in sorted(KINDS)]
    for q in live:
        q.run(2)
    b.close()                                        # soccer_destroy: waits for the stream, frees what is left
    assert all(q.q is None for q in live)
    for q in live:
        q.close()                                    # the wrappers know: no call on a closed handle
    b2 = batch()                                     # the device is as usable as before
    try:
        assert KINDS["wolf_phc"][0](b2).run(1).steps == 1
    finally:
        b2.close()
