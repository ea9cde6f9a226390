"""The host build of the launch plan (csrc/soccer_launch_plan.hpp through tests/host/launch_plan_host.cpp) for
tests/test_launch_plan_host.py (no GPU) and tests/test_gpu_launch_plan.py (-m gpu): the shim's column orders, rows of facts in and
rows of plans out, and the facts a handle of a given pitch and slip contributes, from tests/large_pitch_cases.py classify.
Nothing here looks at a device."""
import ctypes as C
import os
import subprocess

import numpy as np

import large_pitch_cases as lp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HANDLE = ("swar_ok", "slip", "slip_swar_ok", "slip_lut", "slip_step_lut", "small", "wide", "lut_lds", "policy_a", "policy_b", "step_stats",
          "slip_int_one", "stream_actions", "capturing", "worklist", "E", "rollout_pref", "nS", "lane_phase", "smem_bytes", "lds_limit", "n")
STEP_CALL = ("dword_io", "u_step", "u_reset", "u_aligned16", "last_return", "last_return_aligned4", "full", "gym", "worklist_refused")
LAUNCH = ("family", "out", "slipm", "geo", "policy", "expl", "explicit_u", "vec", "shared", "int_only", "slip", "wide", "exact_tail", "act_stream")
STEP_PLAN = ("n4",) + tuple("main_" + k for k in LAUNCH) + tuple("rest_" + k for k in LAUNCH) + ("fusable",)
ROLLOUT_CALL = ("sample_actions", "mix_a", "mix_b", "act_a", "act_b", "full", "hist", "io_width", "parts", "chunks")
ROLLOUT_PLAN = ("refused", "swar", "E", "dyn", "dm", "sm", "geo", "full", "stats", "lds_tables", "tab_off", "act_off", "smem", "table_placement",
                "n4", "tail", "slip", "lut_lds")
SHAPE = ("kernel", "tail", "action_source", "slip_selection", "small_pitch", "full", "table_placement", "parts", "chunks", "dynamic_lds_bytes")
RESET_CALL = ("mask", "u_reset", "dword_io")
RESET_PLAN = ("n4", "masked", "slip", "lut_lds")
SWAR, LANE, HOT = 1, 2, 3           # StepFamily


def build(tmp_dir):
    """compiles the shim with the line of tests/test_policy_rows_host.py -> the three plan functions as rows -> rows"""
    so = os.path.join(str(tmp_dir), "liblaunch_plan_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           "-o", so, os.path.join(ROOT, "tests", "host", "launch_plan_host.cpp")])
    L = C.CDLL(so)

    def rows_to_rows(name, n_in, n_out):
        fn = getattr(L, name)
        fn.restype = None
        fn.argtypes = [C.c_long, C.c_void_p, C.c_void_p]

        def call(rows):
            rows = np.ascontiguousarray(rows, np.int64).reshape(-1, n_in)
            out = np.zeros((len(rows), n_out), np.int64)
            fn(len(rows), rows.ctypes.data, out.ctypes.data)
            return out
        return call
    return dict(step=rows_to_rows("plan_step_host", len(HANDLE) + len(STEP_CALL), len(STEP_PLAN)),
                rollout=rows_to_rows("plan_rollout_host", len(HANDLE) + len(ROLLOUT_CALL), len(ROLLOUT_PLAN) + len(SHAPE)),
                reset=rows_to_rows("plan_reset_host", len(HANDLE) + len(RESET_CALL), len(RESET_PLAN)))


def row(names, **values):
    """one row in the order `names`, what is not given 0"""
    assert set(values) <= set(names), set(values) - set(names)
    return [int(values.get(k, 0)) for k in names]


def handle_facts(width, height, slip, n, lds_limit, **more):
    """what a default handle of this pitch contributes (soccer_create): the byte arithmetic, the layout, the geometry and the
    observation table's place from classify; a slip of these suites (0, or one with an exact integer decision and both table
    forms of the selection, as 0.2 has)"""
    c = lp.classify(width, height)
    f = dict(swar_ok=c["fits"], slip=slip != 0.0, slip_swar_ok=slip != 0.0, slip_lut=slip != 0.0, slip_step_lut=slip != 0.0, small=c["small"],
             wide=not c["packs"], lut_lds=c["lut_lds"], E=4, nS=c["nS"], smem_bytes=c["lds_bytes"], lds_limit=lds_limit, n=n)
    f.update(more)
    return f


def rollout_call(source, extras, steps, n, launch_lanes=1 << 30, hist=True, io_width=4):
    """the call facts of a rollout of tests/rollout_shape_cases.py SOURCES; the launch loops' counts as the launcher makes them"""
    from rollout_shape_cases import SOURCES
    sample, use_a, use_b, fixed = SOURCES[source]
    return dict(sample_actions=sample, mix_a=use_a, mix_b=use_b, act_a=not sample and fixed != "player_a", act_b=not sample and fixed != "player_b",
                full=extras, hist=hist, io_width=io_width, parts=-(-(n & ~3) // launch_lanes), chunks=-(-steps // 4096))


def rollout_shape(plan, facts, call):
    """the plan of one rollout read as SoccerBatch.rollout_shape() gives it -> (shape dict, plan dict)"""
    out = plan["rollout"](row(HANDLE, **facts) + row(ROLLOUT_CALL, **call))[0]
    sh = dict(zip(SHAPE, (int(v) for v in out[len(ROLLOUT_PLAN):])), lds_limit=facts["lds_limit"])
    return sh, dict(zip(ROLLOUT_PLAN, (int(v) for v in out[:len(ROLLOUT_PLAN)])))
