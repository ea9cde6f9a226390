"""What SoccerBatch.rollout_shape() must report for a call's arguments, shared by the suites that launch rollouts
(tests/test_gpu_rollout_action_sources.py, tests/test_gpu_pitch_boundaries.py) and by the CPU test of the launch plan
(tests/test_launch_plan_host.py), which holds the plan, read as a shape, to the same check.  Nothing here looks at a device."""
BYTE_PARALLEL, PER_LANE = 1, 2
NONE, LDS, GLOBAL = 0, 1, 2
SLIP_TABLE_BYTES = (4096 + 40) * 4          # static LDS of the table form of the slip selection
STAGING_BYTES = 16 * 256 * 4                # sixteen dwords per thread when an action stream is read
SLIP_ROWS_BYTES = 36 * 4

# action sources: (sampled in the kernel, mix_a, mix_b, fixed side)
SOURCES = {
    "uniform":            (True, False, False, None),
    "both_mixed":         (True, True, True, None),
    "mix_a":              (True, True, False, None),
    "mix_b":              (True, False, True, None),
    "fixed_a_stream_b":   (False, False, False, "player_a"),
    "fixed_b_stream_a":   (False, False, False, "player_b"),
    "fixed_a_uniform_b":  (True, False, False, "player_a"),
    "fixed_b_mix_a":      (True, True, False, "player_b"),
}


def _table_bytes(nS, source):
    """(bytes of the observation-keyed tables in LDS, the action_source the launch then has / has without them in LDS)"""
    sample, use_a, use_b, fixed = SOURCES[source]
    if source == "uniform":
        return 0, 1, 1
    if source == "both_mixed":
        return 16 * nS, 2, 3
    dm = 4 if source == "fixed_a_stream_b" else 5 if source == "fixed_b_stream_a" else 3
    return 2 * 8 * nS + 2 * ((nS + 15) & ~15), dm, dm


def _check_shape(sh, nS, n, steps, source, kernel, slip_sel, extras, launch_lanes=1 << 30):
    """what rollout_shape() reports against the call's arguments; the placement follows from the reported lds_limit"""
    sample, use_a, use_b, fixed = SOURCES[source]
    tables = source != "uniform"
    assert sh["kernel"] == kernel and sh["chunks"] == -(-steps // 4096) and sh["full"] == int(extras)
    assert sh["slip_selection"] == slip_sel
    if kernel == PER_LANE:
        assert sh["action_source"] == 3 and sh["tail"] == 0 and sh["parts"] == 1
        assert sh["table_placement"] == (GLOBAL if tables else NONE)
        return
    assert sh["tail"] == int(n % 4 != 0) and sh["parts"] == -(-(n & ~3) // launch_lanes)
    staging = 0 if sample else STAGING_BYTES
    static = SLIP_TABLE_BYTES if slip_sel == 2 else 0
    need, dm_lds, dm_global = _table_bytes(nS, source)
    # the tables go to LDS when they fit the limit next to the slip rows, the staging area (+ 16 B to align it) and the slip table
    fits = tables and SLIP_ROWS_BYTES + need + (staging + 16 if staging else 0) + static <= sh["lds_limit"]
    assert sh["table_placement"] == (NONE if not tables else LDS if fits else GLOBAL)
    assert sh["action_source"] == (dm_lds if fits else dm_global)
    tab = SLIP_ROWS_BYTES + (need if fits else 0)
    assert sh["dynamic_lds_bytes"] == (((tab + 15) & ~15) + staging if staging else tab)
    assert sh["dynamic_lds_bytes"] + static <= sh["lds_limit"]
