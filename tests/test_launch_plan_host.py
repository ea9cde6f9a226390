"""CPU: which kernel a call launches, from the compiled plan (csrc/soccer_launch_plan.hpp through tests/host/launch_plan_host.cpp).

  step      every combination of the facts against a restatement of launch_one_step / launch_step as they stood before the plan
            existed (bd59368), written here from that source
  rollout   the action sources of tests/rollout_shape_cases.py at an LDS limit on each side of every table size, through that
            module's _check_shape; the edges of the lane count, the alignment, SOCCER_ROLLOUT=1 and the refusal
  pitches   all 278 accepted pitches against tests/large_pitch_cases.py classify
  reach     the instantiations the plans name over these enumerations are exactly the ones the library emits"""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import large_pitch_cases as lp  # noqa: E402
import launch_plan_cases as lc  # noqa: E402
from launch_plan_cases import HANDLE, HOT, LANE, LAUNCH, RESET_CALL, RESET_PLAN, ROLLOUT_CALL, ROLLOUT_PLAN, STEP_CALL, STEP_PLAN, SWAR  # noqa: E402
from rollout_shape_cases import (BYTE_PARALLEL, PER_LANE, SLIP_ROWS_BYTES, SLIP_TABLE_BYTES, SOURCES, STAGING_BYTES,  # noqa: E402
                                 _check_shape, _table_bytes)

# what the library emits, by the dispatch code and by the assembly listing of the build (make asm)
EMITTED = dict(step_kernel_swar=90, step_kernel=10, step_kernel_hot=3, rollout_swar_kernel=78, rollout_kernel=24, reset_kernel=4,
               reset_kernel_swar=4)
HUGE = (1 << 34) + 4            # a launch of 2^32 groups: beyond the work list's 32-bit indices


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return lc.build(tmp_path_factory.mktemp("launch_plan_host"))


def _distinct(g, rows, names):
    """the distinct tuples of the columns `names` of g over the selected rows"""
    key = sum(g[k][rows] << (4 * i) for i, k in enumerate(names))         # every value is below 16
    return {tuple((int(v) >> (4 * i)) & 15 for i in range(len(names))) for v in np.unique(key)}


# ---- step --------------------------------------------------------------------------------------------------------------------
def step_handles():
    """every handle a step can meet, as rows of HANDLE: what only a slip handle has is varied on slip handles, the geometry form
    where the byte arithmetic fits; the work list exists, can be allocated, cannot (the allocation fails), or may not be (a
    capture); the action-load flag is passed through, so it alternates -> (rows, worklist_refused per row)"""
    rows, refused = [], []
    for swar_ok, small in ((0, 0), (1, 0), (1, 1)):
        for slip, slip_swar_ok, step_lut, int_one in [(0, 0, 0, 0)] + [(1,) + t for t in itertools.product((0, 1), repeat=3)]:
            for wide, E, phase, (pa, pb), stats, (cap, wl, ref), n in itertools.product(
                    (0, 1), (1, 4, 8), (0, 1), ((0, 0), (1, 0), (0, 1)), (0, 1), ((0, 1, 0), (0, 0, 0), (0, 0, 1), (1, 0, 0)), (3, 4, 7, HUGE)):
                rows.append(lc.row(HANDLE, swar_ok=swar_ok, small=small, slip=slip, slip_swar_ok=slip_swar_ok, slip_step_lut=step_lut,
                                   slip_int_one=int_one, wide=wide, E=E, lane_phase=phase, policy_a=pa, policy_b=pb, step_stats=stats,
                                   stream_actions=len(rows) & 1, capturing=cap, worklist=wl, n=n, nS=761, lds_limit=65536, smem_bytes=2048))
                refused.append(ref)
    return np.array(rows, np.int64), np.array(refused, np.int64)


def step_calls():
    """every call: a stream that is not given counts as aligned"""
    for dword, (us, ur, u16), (lr, lr4), full, gym in itertools.product(
            (0, 1), ((0, 0, 1), (1, 0, 1), (1, 0, 0), (0, 1, 1), (0, 1, 0), (1, 1, 1), (1, 1, 0)), ((0, 1), (1, 1), (1, 0)), (0, 1), (0, 1)):
        yield dict(dword_io=dword, u_step=us, u_reset=ur, u_aligned16=u16, last_return=lr, last_return_aligned4=lr4, full=full, gym=gym)


def parent_launch_step(H, c, vec, n_part):
    """soccer_step.hip launch_step(h, P, io, explicit_u, vec) of bd59368 over rows of handles H (bool / int arrays by name) and one
    call c -> the launch as LAUNCH columns.  `vec` and `n_part` are per row."""
    u_step, u_reset = bool(c["u_step"]), bool(c["u_reset"])
    explicit_u = u_step | u_reset | H["policy_a"] | H["policy_b"]               # launch_one_step
    shared = H["lane_phase"] == 0
    policy_only = explicit_u & (not u_step) & (not u_reset)
    al_ret = bool(c["last_return_aligned4"])
    swar_fit = vec & shared & H["swar_ok"] & (~H["slip"] | H["slip_swar_ok"]) & al_ret
    al_u = bool(c["u_aligned16"])
    expl = explicit_u & ~policy_only & ~H["slip"] & al_u
    # (h->d_worklist || (!h->capturing && ensure_worklist(h))): the allocation fails where the call is told so
    listed = H["worklist"] | (~H["capturing"] & ~H["worklist_refused"])
    expl_slip = (explicit_u & ~policy_only & H["slip"] & u_step & al_u & vec & shared & H["swar_ok"] & al_ret
                 & ((n_part >> 2) < 0xffffffff) & listed)
    swar = ((policy_only | ~explicit_u | expl) & swar_fit) | expl_slip
    out = np.where(bool(c["full"]) | H["step_stats"], 2, 1 if (c["gym"] or c["last_return"]) else 0)
    # SWAR_SLIP, then SWAR_GO
    slipm = np.where(expl_slip, 3, np.where(expl, 0, np.where(~H["slip"], 0, np.where(H["slip_step_lut"], 2, 1))))
    xv = expl_slip | expl
    geo = ~H["wide"] & H["small"]
    lean = (not (c["full"] or c["gym"] or c["last_return"])) & ~H["step_stats"]
    generic = ~swar & explicit_u                    # launch_step3<true, vec && shared, vec && shared>
    hot = ~swar & ~explicit_u & vec & shared & lean
    plain = ~swar & ~explicit_u & ~hot              # launch_step3<false, vec, vec && shared>
    z = np.zeros(len(shared), np.int64)
    cols = dict(family=np.where(swar, SWAR, np.where(hot, HOT, LANE)), out=np.where(swar, out, z), slipm=np.where(swar, slipm, z),
                geo=swar & geo, policy=swar & (H["policy_a"] | H["policy_b"]), expl=swar & xv, explicit_u=generic,
                vec=(generic & vec & shared) | (plain & vec), shared=(generic | plain) & vec & shared,
                int_only=hot & H["slip"] & H["slip_int_one"], slip=H["slip"], wide=swar & H["wide"], exact_tail=swar & expl_slip,
                act_stream=swar & H["stream_actions"])
    return np.stack([np.asarray(cols[k], np.int64) for k in LAUNCH], 1)


def parent_launch_one_step(H, c):
    """launch_one_step of bd59368 -> rows of STEP_PLAN without its last column"""
    vec = (H["E"] != 1) & bool(c["dword_io"])
    n = H["n"]
    n4 = np.where(vec, n & ~3, 0)
    main = parent_launch_step(H, c, np.ones(len(n), bool), n4) * (n4 > 0)[:, None]
    rest = parent_launch_step(H, c, np.zeros(len(n), bool), n - n4) * (n4 < n)[:, None]
    return np.concatenate([n4[:, None], main, rest], 1)


@pytest.fixture(scope="module")
def step_sweep(plan):
    """every step plan once: what differs from the restatement, which invariants break, and the instantiations named (the
    reachable-set test reads them, so it runs alone as well as after the step test)"""
    rows, refused = step_handles()
    H = {k: (rows[:, i] != 0 if k not in ("E", "n", "lane_phase", "nS", "smem_bytes", "lds_limit", "rollout_pref") else rows[:, i])
         for i, k in enumerate(HANDLE)}
    H["worklist_refused"] = refused != 0
    col = {k: i for i, k in enumerate(STEP_PLAN)}
    named = dict(step_kernel_swar=set(), step_kernel=set(), step_kernel_hot=set())
    differ, broken, total, fused = [], [], 0, 0
    for c in step_calls():
        call = np.tile(lc.row(STEP_CALL, **c), (len(rows), 1))
        call[:, STEP_CALL.index("worklist_refused")] = refused
        got = plan["step"](np.concatenate([rows, call], 1))
        bad = (got[:, :-1] != parent_launch_one_step(H, c)).any(1)
        if bad.any():
            differ.append((c, dict(zip(HANDLE, rows[bad][0].tolist())), int(bad.sum())))
        total += len(rows)
        listable = H["worklist"] | (~H["capturing"] & ~H["worklist_refused"])
        for part in ("main_", "rest_"):
            g = {k: got[:, col[part + k]] for k in LAUNCH}
            fam = g["family"]
            exists = got[:, col["n4"]] > 0 if part == "main_" else got[:, col["n4"]] < H["n"]
            holds = {"exactly one family": (np.isin(fam, (SWAR, LANE, HOT)) == exists) & ((fam == 0) | exists),
                     "SLIPM 3 with EXPL and a work list": (g["slipm"] != 3) | ((g["expl"] == 1) & listable),
                     "SLIPM 3 with the exact walk": (g["slipm"] == 3) == (g["exact_tail"] == 1),
                     "the wide layout with GEO 0": (g["wide"] == 0) | (g["geo"] == 0)}
            broken += [(what, part, c) for what, ok in holds.items() if not ok.all()]
            named["step_kernel_swar"] |= _distinct(g, fam == SWAR, ("out", "slipm", "policy", "geo", "expl", "wide"))
            named["step_kernel"] |= _distinct(g, fam == LANE, ("slip", "explicit_u", "vec", "shared"))
            if (g["exact_tail"] == 1).any():
                named["step_kernel"].add((1, 1, 1, 1))
            named["step_kernel_hot"] |= _distinct(g, fam == HOT, ("slip", "int_only"))
        # a step that may join a fused run is, alone, the byte-parallel kernel with the four result streams, or with the histogram
        fus = got[:, col["fusable"]] == 1
        out = got[fus, col["main_out"]]
        if not ((got[fus, col["n4"]] == H["n"][fus]) & (got[fus, col["main_family"]] == SWAR) & np.isin(out, (0, 2))
                & ((out == 2) == H["step_stats"][fus])).all():
            broken.append(("fusable: byte-parallel with OUT 0, or OUT 2 only under step statistics", "main_", c))
        fused += int(fus.sum())
    return dict(named=named, differ=differ, broken=broken, total=total, fused=fused, handles=len(rows))


def test_step_plans_are_the_parent_s_over_every_combination_of_the_facts(step_sweep):
    w = step_sweep
    print("%d handles x %d calls = %d step plans, %d of them fusable" % (w["handles"], w["total"] // w["handles"], w["total"], w["fused"]))
    assert w["differ"] == [], "plans that are not the restatement's (call, first handle, rows): %s" % w["differ"][:3]
    assert w["broken"] == []
    assert w["total"] > 10000 and w["fused"] > 0


# ---- rollout -----------------------------------------------------------------------------------------------------------------
def _fixed(source):
    return dict(policy_a=SOURCES[source][3] == "player_a", policy_b=SOURCES[source][3] == "player_b")


def _limits(nS, source, slip_sel):
    """an LDS limit at which the source's tables just fit, and one byte less; the device's two real limits"""
    need = _table_bytes(nS, source)[0]
    staging = 0 if SOURCES[source][0] else STAGING_BYTES + 16
    exact = SLIP_ROWS_BYTES + need + staging + (SLIP_TABLE_BYTES if slip_sel == 2 else 0)
    return sorted({exact, exact - 1, 64 * 1024, 160 * 1024} if need else {64 * 1024, 160 * 1024})


PITCHES = ((5, 4), (7, 6), (9, 6), (10, 7), (11, 7))         # of tests/test_gpu_rollout_action_sources.py CASES: nS 761 .. 11705


@pytest.mark.parametrize("source", sorted(SOURCES))
def test_rollout_plans_pass_the_gpu_suite_s_shape_check_on_each_side_of_each_table_size(plan, source):
    met = set()
    for (w, h), slip_sel, extras, n in itertools.product(PITCHES, (0, 1, 2), (False, True), (3, 4, 7, 4096 + 3)):
        nS = lp.classify(w, h)["nS"]
        for limit in _limits(nS, source, slip_sel):
            f = lc.handle_facts(w, h, 0.2 if slip_sel else 0.0, n, limit, slip_lut=slip_sel == 2, **_fixed(source))
            sh, p = lc.rollout_shape(plan, f, lc.rollout_call(source, extras, 48, n))
            kernel = BYTE_PARALLEL if n >= 4 else PER_LANE            # fewer than four lanes: the per-lane kernel
            _check_shape(sh, nS, n, 48, source, kernel, slip_sel if n >= 4 else int(slip_sel != 0), extras)
            assert not p["refused"] and p["swar"] == (n >= 4) and p["n4"] == (n & ~3 if n >= 4 else 0) and p["tail"] == (n >= 4 and n % 4 != 0)
            assert p["stats"] == 1 and p["dyn"] == 1 and p["geo"] == (lp.classify(w, h)["small"] if n >= 4 else 0)
            if n >= 4:
                assert p["tab_off"] == 36 and p["act_off"] * 4 == (0 if SOURCES[source][0] else sh["dynamic_lds_bytes"] - STAGING_BYTES)
                met.add((sh["table_placement"], limit))
    if source != "uniform":
        assert {pl for pl, _ in met} == {1, 2}                      # LDS and global memory were both met


def test_rollout_plan_edges(plan):
    f = lc.handle_facts(5, 4, 0.2, 4096, 160 * 1024)
    streams = dict(act_a=1, act_b=1, hist=1, io_width=4, parts=1, chunks=1)
    sh, p = lc.rollout_shape(plan, f, streams)
    assert (p["swar"], p["dm"], p["sm"], p["geo"], p["stats"], p["smem"]) == (1, 0, 2, 1, 1, SLIP_ROWS_BYTES + STAGING_BYTES)
    # a misaligned stream: the per-lane kernel at the widest E the streams allow
    for E, width, want in ((8, 8, 8), (8, 4, 4), (8, 1, 1), (4, 8, 4), (4, 4, 4), (4, 1, 1), (1, 8, 1), (1, 1, 1)):
        sh, p = lc.rollout_shape(plan, dict(f, E=E, rollout_pref=1), dict(streams, io_width=width))
        assert (p["swar"], p["E"], p["dyn"], sh["kernel"], sh["dynamic_lds_bytes"]) == (0, want, 0, PER_LANE, f["smem_bytes"])
        sh, p = lc.rollout_shape(plan, dict(f, E=E), dict(streams, io_width=width))
        assert p["swar"] == (width >= 4) and (p["swar"] or p["E"] == want)
    # SOCCER_ROLLOUT=1, a lane offset off the phase, a slip without an exact integer decision, a pitch beyond the byte arithmetic
    for change in (dict(rollout_pref=1), dict(lane_phase=2), dict(slip_swar_ok=0), dict(swar_ok=0), dict(n=3)):
        sh, p = lc.rollout_shape(plan, dict(f, **change), dict(streams, full=1))
        assert (p["swar"], p["E"], sh["kernel"], sh["slip_selection"], sh["full"], sh["parts"], sh["tail"]) == (0, 4, PER_LANE, 1, 1, 1, 0)
    assert lc.rollout_shape(plan, dict(f, rollout_pref=2), streams)[1]["swar"] == 1
    # the tail: the per-lane kernel at E = 1 over n & 3 lanes
    for n in (4, 7):
        sh, p = lc.rollout_shape(plan, dict(f, n=n), streams)
        assert (p["swar"], p["n4"], p["tail"], p["E"], sh["tail"]) == (1, 4, int(n == 7), 1, int(n == 7))
    # hist == nullptr: only the shape of a fused run of captured steps
    unread = dict(streams, hist=0)
    sh, p = lc.rollout_shape(plan, f, unread)
    assert (p["refused"], p["swar"], p["stats"], p["dm"], p["full"]) == (0, 1, 0, 0, 0)
    for facts, call in ((dict(f, n=4099), unread), (dict(f, rollout_pref=1), unread), (f, dict(unread, full=1)), (dict(f, policy_a=1), unread),
                        (dict(f, policy_b=1), unread), (f, dict(unread, sample_actions=1)), (f, dict(unread, io_width=1))):
        assert lc.rollout_shape(plan, facts, call)[1]["refused"] == 1
        assert lc.rollout_shape(plan, facts, dict(call, hist=1))[1]["refused"] == 0


# ---- pitches -----------------------------------------------------------------------------------------------------------------
def test_plans_use_fits_packs_small_and_lut_lds_as_classify_does_on_every_accepted_pitch(plan):
    accepted = [(w, h) for w in range(5, 121) for h in range(4, 121) if lp.refusal(w, h) is None]
    assert len(accepted) == 278
    step = {k: i for i, k in enumerate(STEP_PLAN)}
    for (w, h), slip in itertools.product(accepted, lp.SLIPS):
        c = lp.classify(w, h)
        f = lc.handle_facts(w, h, slip, lp.N, 160 * 1024)
        sh, p = lc.rollout_shape(plan, f, dict(act_a=1, act_b=1, hist=1, io_width=4, parts=1, chunks=1))
        assert p["swar"] == c["fits"] and sh["small_pitch"] == c["small"] and p["geo"] == c["small"]
        assert sh["dynamic_lds_bytes"] == (SLIP_ROWS_BYTES + STAGING_BYTES if c["fits"] else c["lds_bytes"])
        s = plan["step"](lc.row(HANDLE, **f) + lc.row(STEP_CALL, dword_io=1, u_aligned16=1, last_return_aligned4=1))[0]
        assert s[step["n4"]] == lp.N & ~3 and s[step["main_family"]] == (SWAR if c["fits"] else HOT) and s[step["rest_family"]] == LANE
        assert s[step["main_wide"]] == (c["fits"] and not c["packs"]) and s[step["main_geo"]] == (c["small"] and c["packs"])
        r = dict(zip(RESET_PLAN, plan["reset"](lc.row(HANDLE, **f) + lc.row(RESET_CALL, dword_io=1))[0]))
        assert r == dict(n4=(lp.N & ~3) if c["fits"] else 0, masked=0, slip=slip != 0.0, lut_lds=c["lut_lds"])


# ---- the reachable set -------------------------------------------------------------------------------------------------------
def test_the_plans_name_exactly_the_emitted_instantiations(plan, step_sweep):
    """the step's instantiations from the sweep of every step plan; here every rollout and reset over small sets of every fact.
    The counts are compared with EMITTED and every name with the shapes the kernels are compiled for (their static_asserts and
    the launchers' `if constexpr`), not with the symbol names of the assembly listing: tools/asm_compare.py does that per build."""
    _NAMED = dict(step_sweep["named"], rollout_swar_kernel=set(), rollout_kernel=set(), reset_kernel=set(), reset_kernel_swar=set())
    calls = [lc.row(ROLLOUT_CALL, sample_actions=s, mix_a=ma, mix_b=mb, act_a=aa, act_b=ab, full=fl, hist=1, io_width=wd, parts=1, chunks=1)
             for s, ma, mb, aa, ab, fl, wd in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (1, 4, 8))]
    calls.append(lc.row(ROLLOUT_CALL, act_a=1, act_b=1, hist=0, io_width=4, parts=1, chunks=1))      # a fused run without step statistics
    calls = np.array(calls, np.int64)
    col = {k: i for i, k in enumerate(ROLLOUT_PLAN)}
    for swar_ok, small, (slip, slip_ok, lut), lut_lds, (pa, pb), E, limit, n in itertools.product(
            (0, 1), (0, 1), ((0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)), (0, 1), ((0, 0), (1, 0), (0, 1), (1, 1)), (1, 4, 8), (20000, 65536),
            (4, 7)):
        f = lc.row(HANDLE, swar_ok=swar_ok, small=small and swar_ok, slip=slip, slip_swar_ok=slip_ok, slip_lut=lut, lut_lds=lut_lds, policy_a=pa,
                   policy_b=pb, E=E, nS=761, lds_limit=limit, smem_bytes=2048, n=n)
        got = plan["rollout"](np.concatenate([np.tile(f, (len(calls), 1)), calls], 1))
        got = got[got[:, col["refused"]] == 0]
        g = {k: got[:, i] for k, i in col.items()}
        s = g["swar"] == 1
        _NAMED["rollout_swar_kernel"] |= _distinct(g, s, ("dm", "sm", "geo", "full", "stats"))
        assert (g["slip"] == slip).all() and (g["lut_lds"] == lut_lds).all()
        _NAMED["rollout_kernel"] |= _distinct(g, ~s, ("E", "slip", "lut_lds", "dyn"))               # E = 1 where it is a tail
        _NAMED["rollout_kernel"] |= _distinct(g, s & (g["tail"] == 1), ("E", "slip", "lut_lds", "dyn"))
        for mask, u_reset, dword, phase in itertools.product((0, 1), repeat=4):
            r = plan["reset"](f[:HANDLE.index("lane_phase")] + [phase] + f[HANDLE.index("lane_phase") + 1:] + [mask, u_reset, dword])[0]
            if r[0]:
                _NAMED["reset_kernel_swar"].add((int(r[1]), int(r[2])))
            if r[0] < n:
                _NAMED["reset_kernel"].add((int(r[3]), int(r[2])))
    assert {k: len(v) for k, v in _NAMED.items()} == EMITTED
    # ... and none outside the shapes the kernels are compiled for
    assert all((sm == 3) <= bool(x) and (not x or sm in (0, 3)) and not (wide and geo) for _, sm, _, geo, x, wide in _NAMED["step_kernel_swar"])
    assert all(stats or (dm == 0 and not full) for dm, _, _, full, stats in _NAMED["rollout_swar_kernel"])
    assert all(slip or not int_only for slip, int_only in _NAMED["step_kernel_hot"])
    assert {(e, v, s) for _, e, v, s in _NAMED["step_kernel"]} == {(1, 1, 1), (1, 0, 0), (0, 1, 1), (0, 1, 0), (0, 0, 0)}
