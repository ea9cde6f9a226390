"""The pitches at every boundary of the environment's kernel dispatch, defined once for tests/test_pitch_boundaries_np.py (no GPU)
and tests/test_gpu_pitch_boundaries.py (-m gpu), with the four host-side predicates that choose a handle's kernels restated in
Python from the headers:

  fits     csrc/soccer_swar.hpp swar::fits      byte-parallel kernels or per-lane kernels
  packs    csrc/soccer_swar.hpp swar::packs     three packed state streams or six
  small    csrc/soccer_swar.hpp make_consts     byte tables (GEO = 1) or arithmetic geometry
  lut_lds  csrc/soccer_hip.hip soccer_create    the observation table staged in LDS or read from global memory

and the size refusals of csrc/soccer_rules.hpp Rules::build.  W is the width plus the two goal columns, NI = H * (W - 2) the
interior cells, nS = 2 * NI * (NI - 1) + 1 the observation indices.  Nothing here looks at a device."""
import numpy as np

LDS_LINE = 150 * 1024           # soccer_create: what the tables of the per-lane kernels may take of a workgroup's LDS
ISD_WORDS = 16                  # csrc/soccer_kernels.hpp kIsdWords: four kick-offs of four words
MAX_STEPS = 20                  # of every handle of these suites: episodes truncate inside a rollout of T steps
T = 48
N, STRIDE = 4096 + 3, 4096 + 4  # rollouts: a ragged tail, rows a multiple of 4 apart
SLIPS = (0.0, 0.2)


def refusal(width, height):
    """Rules::build: the message with which a pitch is refused, None where it is accepted"""
    if width < 5: return "Width must be at least 5 columns."
    if height < 4: return "Height must be at least 4 rows."
    if height > 120 or width > 120: return "pitch too large (rows/cols must fit int8)"
    H, W = height, width + 2
    if 2 * H * W * H * W > 1 << 24: return "pitch too large (tuple table)"
    NI = H * (W - 2)
    if 2 * NI * (NI - 1) + 1 > 0xFFFE: return "pitch too large (observation index must fit uint16)"
    if (2 * H * W * 5 + ISD_WORDS) * 4 > LDS_LINE: return "pitch too large: the move/bounds table"     # soccer_create; never met
    return None


def classify(width, height, max_steps=MAX_STEPS):
    """what soccer_create decides for an accepted pitch"""
    assert refusal(width, height) is None, (width, height)
    H, W = height, width + 2
    NI = H * (W - 2)
    fits = H >= 4 and W >= 7 and H * W <= 128 and 2 * NI + 2 <= 255 and 1 <= max_steps <= 127
    nc_bytes = (2 * H * W * 5 + ISD_WORDS) * 4                  # the move/bounds table and the kick-off words
    lut_bytes = 2 * H * W * H * W * 2                           # one uint16 per tuple
    lut_lds = nc_bytes + lut_bytes <= LDS_LINE
    return dict(w=width, h=height, W=W, H=H, NI=NI, nS=2 * NI * (NI - 1) + 1, kickoffs=4 if H % 2 == 0 else 2,
                fits=fits, packs=H <= 8 and W <= 16, small=fits and H + 2 <= 8 and W <= 8, lut_lds=lut_lds,
                nc_bytes=nc_bytes, lut_bytes=lut_bytes, lds_bytes=nc_bytes + (lut_bytes if lut_lds else 0))


# name -> (width, height), what the row claims: (fits, packs, small, lut_lds), kick-offs, nS,
#         the neighbour on the other side of a predicate: (width, height, predicate) or None
_ROWS = [
    ("6x6",   (6, 6),   (True, True, True, True),     4, 2521,  (6, 7, "small")),       # last small: W = 8, H + 2 = 8
    ("6x7",   (6, 7),   (True, True, False, True),    2, 3445,  (6, 6, "small")),       # first not small by height
    ("14x8",  (14, 8),  (True, True, False, True),    4, 24865, (15, 8, "fits")),       # last packs and last fits: row 7, column 15
    ("15x8",  (15, 8),  (False, False, False, True),  4, 28561, (14, 8, "packs")),      # first past both
    ("15x4",  (15, 4),  (True, False, False, True),   4, 7081,  (14, 4, "packs")),      # first long pitch that does not pack
    ("30x4",  (30, 4),  (True, False, False, True),   4, 28561, (31, 4, "fits")),       # last long pitch that fits: column 31
    ("31x4",  (31, 4),  (False, False, False, True),  4, 30505, (30, 4, "fits")),
    ("5x9",   (5, 9),   (True, False, False, True),   2, 3961,  (5, 8, "packs")),       # first tall pitch that does not pack
    ("5x18",  (5, 18),  (True, False, False, True),   4, 16021, (5, 19, "fits")),       # last tall pitch that fits: row 17
    ("5x19",  (5, 19),  (False, False, False, True),  2, 17861, (5, 18, "fits")),
    ("12x14", (12, 14), (False, False, False, False), 4, 56113, (13, 9, "lut_lds")),    # table in global memory; 13x9 is the suites' other per-lane pitch
    ("36x5",  (36, 5),  (False, False, False, True),  2, 64441, (30, 6, "lut_lds")),    # the largest LDS request under the line
    ("45x4",  (45, 4),  (False, False, False, True),  4, 64441, (30, 6, "lut_lds")),    # the largest nS with the table in LDS: column 46
    ("30x6",  (30, 6),  (False, False, False, False), 4, 64441, (36, 5, "lut_lds")),    # the largest nS with the table in global memory
    ("5x36",  (5, 36),  (False, False, False, False), 4, 64441, (45, 4, "lut_lds")),    # rows to 35, a 254 016 B table
]
CASES = {name: dict(classify(*wh), name=name, claim=dict(zip(("fits", "packs", "small", "lut_lds"), claim)), claim_kickoffs=k, claim_nS=nS,
                    neighbour=nb) for name, wh, claim, k, nS, nb in _ROWS}
NAMES = [r[0] for r in _ROWS]
LARGEST_LDS, LARGEST_NS = 152064, 64441          # 36x5's request; NI = 180 (NI = 181 is prime: no pitch has it)
ACCEPTED_AT_THE_LIMIT = ("45x4", "36x5", "30x6", "5x36")
REFUSED = [((13, 14), "observation index must fit uint16"), ((26, 7), "observation index must fit uint16"),
           ((121, 4), "must fit int8"), ((5, 121), "must fit int8"), ((120, 120), "tuple table"),
           ((4, 4), "Width must be at least 5 columns."), ((5, 3), "Height must be at least 4 rows.")]


def goal_rows(H):
    """Rules::build: the two middle rows of an even height, the three of an odd one"""
    return [(H - 1) // 2, H // 2] if H % 2 == 0 else [H // 2 - 1, H // 2, H // 2 + 1]


def tuples_of(o, kinds):
    """int64[n, 5] (row_a, col_a, row_b, col_b, poss) of the oracle's tuples of the given kinds (1 live, 2 goal), in table order"""
    kind = o.tables()[1]
    f = np.flatnonzero(np.isin(kind, kinds))
    p = f & 1; r = f >> 1
    cb = r % o.W; r //= o.W; rb = r % o.H; r //= o.H; ca = r % o.W; ra = r // o.W
    return np.stack([ra, ca, rb, cb, p], 1).astype(np.int64)


def observations(o):
    """the observation index of every lane of an oracle, from its tuple table"""
    f = ((((o.row_a.astype(np.int64) * o.W + o.col_a) * o.H + o.row_b) * o.W + o.col_b) << 1) | (o.poss & 1)
    return o.tables()[0][f]


# ---- (a) the whole transition relation in one step ---------------------------------------------------------------------------
def sweep_lanes(tup):
    """every tuple x the 25 action pairs, one lane each, then lanes repeated from the front until the count is 3 modulo 4, so that
    every step of the handle leaves a ragged tail of three -> (tuple per lane int64[n, 5], act_a int8[n], act_b int8[n])"""
    idx = np.arange(len(tup) * 25)
    idx = np.concatenate([idx, idx[:(3 - len(idx)) % 4]])
    return tup[idx // 25], ((idx % 25) // 5).astype(np.int8), (idx % 5).astype(np.int8)


def sweep_floors(c):
    """what one step of the sweep must show at the least, from the pitch alone: a carrier next to a goal mouth walks in with one of
    the five actions whatever the other player does (5 action pairs x the other's cells, far more than 100 lanes on every case),
    and with t = max_steps - 1 every lane that does not score truncates"""
    return dict(plus=100, minus=100, truncated=20 * c["nS"])


def reach_of_step(c, st, out):
    """what an oracle step from the tuples st showed: the largest row and column a player stood on, the largest observation
    returned as obs and as final_obs, episodes ended by sign, truncations"""
    return dict(row=int(max(st[:, 0].max(), st[:, 2].max())), col=int(max(st[:, 1].max(), st[:, 3].max())),
                obs=int(out["obs"].max()), final_obs=int(out["final_obs"].max()), plus=int((out["reward"] == 1).sum()),
                minus=int((out["reward"] == -1).sum()), truncated=int(((out["truncated"] != 0) & (out["terminated"] == 0)).sum()))


# ---- (b) rollouts -----------------------------------------------------------------------------------------------------------
# of the 4099 lanes 1021 start next to a goal mouth with the ball (a fifth of their first actions walks in: about 100 episodes of
# each sign at step 0 alone) and 2041 at a timestep drawn from 0 .. 19 (each truncates within 20 steps unless it scores first)
ROLLOUT_FLOORS = dict(plus=100, minus=100, truncated=2000)


def rollout_start(o, rng):
    """the state a rollout of these suites starts from, as set_state arguments, for an oracle (and a handle) that was just reset:
    lanes 1 and 6 on the tuple numbered nS - 1 and lane 2 on the one numbered 1 (what _start_on_the_boundary_rows of
    tests/test_gpu_rollout_action_sources.py does), lanes 8 .. 15 with a player on the last row and the last interior column,
    every fourth lane from 16 on next to a goal mouth with the ball, every other lane from 17 on a live tuple drawn uniformly at a
    timestep drawn from 0 .. max_steps - 1; the rest stay on the kick-off the reset gave them."""
    n = o.n
    lut, kind = o.tables()[:2]
    live = tuples_of(o, [1])
    st = dict(row_a=o.row_a.astype(np.int64), col_a=o.col_a.astype(np.int64), row_b=o.row_b.astype(np.int64), col_b=o.col_b.astype(np.int64),
              poss=(o.poss & 1).astype(np.int64), t=o.t.astype(np.int64))

    def put(lanes, tup, t=None):
        for k, name in enumerate(("row_a", "col_a", "row_b", "col_b", "poss")):
            st[name][lanes] = tup[:, k]
        if t is not None:
            st["t"][lanes] = t
    put(np.array([1, 6, 2]), live[[len(live) - 1, len(live) - 1, 0]])       # live tuples are numbered in table order: 1 .. nS - 1
    corner = live[((live[:, 0] == o.H - 1) & (live[:, 1] == o.W - 2)) | ((live[:, 2] == o.H - 1) & (live[:, 3] == o.W - 2))]
    put(np.arange(8, 16), corner[rng.integers(0, len(corner), 8)])
    spread = np.arange(17, n, 2)
    put(spread, live[rng.integers(0, len(live), len(spread))], rng.integers(0, MAX_STEPS, len(spread)))
    ccol = np.where(live[:, 4] == 0, live[:, 1], live[:, 3]); crow = np.where(live[:, 4] == 0, live[:, 0], live[:, 2])
    near = live[np.isin(ccol, [1, o.W - 2]) & np.isin(crow, goal_rows(o.H))]
    mouth = np.arange(16, n, 4)
    put(mouth, near[rng.integers(0, len(near), len(mouth))])
    out = {k: v.astype(np.uint8 if k in ("poss", "t") else np.int8) for k, v in st.items()}
    out["needs_reset"] = np.zeros(n, np.uint8)
    return out


def streamed_run(o, acts):
    """len(acts) oracle steps on streamed actions -> what the run saw, as rollout floors are stated"""
    seen = dict(row=0, col=0, obs=0, final_obs=0, plus=0, minus=0, truncated=0)
    for a in acts:
        seen["row"] = max(seen["row"], int(o.row_a.max()), int(o.row_b.max())); seen["col"] = max(seen["col"], int(o.col_a.max()), int(o.col_b.max()))
        c = o.step(a[0], a[1])
        seen["obs"] = max(seen["obs"], int(c["obs"].max())); seen["final_obs"] = max(seen["final_obs"], int(c["final_obs"].max()))
        seen["plus"] += int((c["reward"] == 1).sum()); seen["minus"] += int((c["reward"] == -1).sum())
        seen["truncated"] += int(((c["truncated"] != 0) & (c["terminated"] == 0)).sum())
    return seen
